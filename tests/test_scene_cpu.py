"""CPU checks of the scene layer (include/oi_scene.h; oi_amd.scene): header <=> library <=> binding, the
C ABI's refusals (checked on the host before any launch), the Python refusals, the default window proved by brute force in
float64, the self-consistency of the restatement the GPU tests compare against (tests/helpers/scene_ref.py), and the
CONDITIONS the GPU tests' inputs must satisfy on the float64 closed form / the oracle alone: the exclusion caps of the
analytic two-sphere scene and of the golden two-instance scene, no ray on the cull's edge, some points shadowed by the other
sphere."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import scene_ref as SR
from helpers import trace_ref as T

ENTRIES = ["oi_scene_begin", "oi_scene_points", "oi_scene_resolve", "oi_scene_shade", "oi_scene_shadow_begin", "oi_scene_visibility",
           "oi_scene_visible"]
R_SCENE = 16                      # the generator of the GPU tests: crop resolution 16, scene resolution 99
GOLDEN_W = 16                     # window of the golden two-instance scene
ORACLE_DEPTH_GAP, ORACLE_CAP = 1e-4, 0.03


def fake_gen(R=R_SCENE):
    """What the host half of oi_amd.scene reads of a Generator: the real camera module and pose prior, no networks."""
    from oi_amd.camera import Camera
    from oi_amd.pose import Plane
    cam_dist, scene_fov, S = T.example_camera(R)
    return types.SimpleNamespace(camera=Camera(cam_dist, scene_fov, S), scene_resolution=S, resolution=R, z_dim=64, it=torch.zeros(1),
                                 pose_prior=Plane([0, -1, 0], 360, [6, 3.5], 20))


_lib = cabi.built_lib


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_scene.h", lib)
    assert sorted(names) == ENTRIES == lib.symbols("oi_scene.h") and mirrors == ["SceneShadeParams"]
    text = cabi.read("oi_scene.h")
    assert int(re.search(r"#define OI_SCENE_MAX_RESOLUTION (\d+)", text).group(1)) == lib.SCENE_MAX_RESOLUTION == 32768
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"scene.hip"' in src and "include/oi_scene.h" in src


def invalid_argument_cases(lib, L, f, arrays=None):
    """(call, entry, text of the message) of the refusals; f: a non-null pointer for every array (never dereferenced: each
    call returns before any launch), arrays: {field: pointer} to use instead for the state."""
    arrays = arrays or {}
    keep = []

    def batch(E=3, N=16, live=f, **kw):
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = N, E, live
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, kw.get(n, arrays.get(n, f)))
        keep.append(b)
        return ctypes.byref(b)

    def shade(**kw):
        P = lib.SceneShadeParams()
        P.E, P.W, P.S, P.L, P.n_pad = kw.get("E", 3), kw.get("W", 4), kw.get("S", 8), kw.get("L", 1), kw.get("n_pad", 5)
        for n, _ in lib.SceneShadeParams._fields_[5:]:
            setattr(P, n, kw.get(n, f))
        keep.append(P)
        return L.oi_scene_shade(ctypes.byref(P), None)

    begin = lambda b=None, c2b=f, W=4, S=8: L.oi_scene_begin(batch() if b is None else b, c2b, f, f, W, S, None)
    resolve = lambda b=None, W=4, S=8, owner=f: L.oi_scene_resolve(batch() if b is None else b, f, W, S, owner, f, None)
    visible = lambda b=None, W=4, S=8, vi=f: L.oi_scene_visible(batch() if b is None else b, f, f, W, S, vi, f, None)
    points = lambda b=None, n_pad=5, n_vis=9, pos=f: L.oi_scene_points(batch() if b is None else b, f, f, n_pad, f, n_vis, f, f, pos, f, f, None)
    sbegin = lambda b=None, n_pad=5, n_vis=8, Lt=2, bias=1e-2, elem=f: L.oi_scene_shadow_begin(
        batch() if b is None else b, f, f, n_pad, f, elem, f, f, n_vis, f, Lt, f, bias, None)
    vis = lambda st=f, E=3, N=16, Lt=2, n_vis=8, S=8, out=f: L.oi_scene_visibility(st, f, f, f, f, E, N, Lt, n_vis, S, out, None)
    return [(lambda: L.oi_scene_begin(None, f, f, f, 4, 8, None), "oi_scene_begin", "null batch"),
            (lambda: begin(batch(E=0)), "oi_scene_begin", "E=0"),
            (lambda: begin(batch(E=1025)), "oi_scene_begin", "E=1025"),
            (lambda: begin(W=5), "oi_scene_begin", "W=5"),
            (lambda: begin(W=0), "oi_scene_begin", "W=0"),
            (lambda: begin(S=0), "oi_scene_begin", "S=0"),
            (lambda: begin(S=32769), "oi_scene_begin", "S=32769"),
            (lambda: begin(batch(E=1024, N=1449 * 1449), W=1449), "oi_scene_begin", "2^31"),
            (lambda: begin(c2b=None), "oi_scene_begin", "null input"),
            (lambda: begin(batch(points=None)), "oi_scene_begin", "null pointer"),
            (lambda: begin(batch(live=None)), "oi_scene_begin", "null live"),
            (lambda: resolve(W=3), "oi_scene_resolve", "W=3"),
            (lambda: resolve(S=-1), "oi_scene_resolve", "S=-1"),
            (lambda: resolve(owner=None), "oi_scene_resolve", "null pointer"),
            (lambda: resolve(batch(E=0)), "oi_scene_resolve", "E=0"),
            (lambda: visible(W=5), "oi_scene_visible", "W=5"),
            (lambda: visible(vi=None), "oi_scene_visible", "null pointer"),
            (lambda: visible(batch(counts=None)), "oi_scene_visible", "null pointer"),
            (lambda: L.oi_scene_shade(None, None), "oi_scene_shade", "null params"),
            (lambda: shade(E=0), "oi_scene_shade", "E=0"),
            (lambda: shade(W=0), "oi_scene_shade", "W=0"),
            (lambda: shade(E=1024, W=1449), "oi_scene_shade", "2^31"),
            (lambda: shade(S=0), "oi_scene_shade", "S=0"),
            (lambda: shade(n_pad=17), "oi_scene_shade", "n_pad=17"),
            (lambda: shade(n_pad=-1), "oi_scene_shade", "n_pad=-1"),
            (lambda: shade(L=0), "oi_scene_shade", "L=0"),
            (lambda: shade(L=257), "oi_scene_shade", "L=257"),
            (lambda: shade(owner=None), "oi_scene_shade", "null owner"),
            (lambda: shade(grad=None), "oi_scene_shade", "null input"),
            (lambda: points(n_pad=0), "oi_scene_points", "n_pad=0"),
            (lambda: points(n_pad=17), "oi_scene_points", "n_pad=17"),
            (lambda: points(n_vis=0), "oi_scene_points", "n_vis=0"),
            (lambda: points(n_vis=16), "oi_scene_points", "n_vis=16"),
            (lambda: points(pos=None), "oi_scene_points", "null pointer"),
            (lambda: sbegin(Lt=0), "oi_scene_shadow_begin", "L=0"),
            (lambda: sbegin(Lt=3), "oi_scene_shadow_begin", "N must be L * n_vis"),
            (lambda: sbegin(n_vis=0, Lt=1), "oi_scene_shadow_begin", "n_vis=0"),
            (lambda: sbegin(n_pad=2), "oi_scene_shadow_begin", "n_pad=2"),
            (lambda: sbegin(bias=-1.0), "oi_scene_shadow_begin", "bias"),
            (lambda: sbegin(elem=None), "oi_scene_shadow_begin", "null input"),
            (lambda: sbegin(batch(E=0)), "oi_scene_shadow_begin", "E=0"),
            (lambda: vis(E=0), "oi_scene_visibility", "E=0"),
            (lambda: vis(N=0), "oi_scene_visibility", "N=0"),
            (lambda: vis(Lt=257), "oi_scene_visibility", "L=257"),
            (lambda: vis(S=0), "oi_scene_visibility", "S=0"),
            (lambda: vis(n_vis=49), "oi_scene_visibility", "n_vis=49"),
            (lambda: vis(E=1024, N=1 << 20, Lt=256, n_vis=1 << 14), "oi_scene_visibility", "2^31"),
            (lambda: vis(out=None), "oi_scene_visibility", "null pointer"),
            (lambda: vis(st=None), "oi_scene_visibility", "null pointer")]


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
    from oi_amd import lib, scene
    gen = fake_gen()
    z = torch.zeros(64)
    centre = T.pose("centre")
    with pytest.raises(ValueError, match=r"1 \.\. 1024 instances"):
        scene.trace_scene(gen, torch.zeros(0, 64), torch.zeros(0, 4, 4))
    with pytest.raises(ValueError, match=r"1 \.\. 1024 instances"):
        scene.trace_scene(gen, torch.zeros(1025, 64), centre[None].expand(1025, 4, 4))
    with pytest.raises(ValueError, match="one pose per latent"):
        scene.trace_scene(gen, [z, z], [centre])
    with pytest.raises(ValueError, match="instance 1 is behind the camera"):
        scene.trace_scene(gen, [z, z], [centre, SR.shifted("centre", 0, 0, -30.0)])
    cam_dist = T.example_camera(R_SCENE)[0]
    with pytest.raises(ValueError, match="instance 2: the camera is inside or within 1"):
        scene.trace_scene(gen, [z] * 3, [centre, centre, SR.shifted("centre", 0, 0, -cam_dist + 1.9)])
    scene.scene_windows(gen, SR.shifted("centre", 0, 0, -cam_dist + 2.1)[None])           # 2.1 from the camera: accepted
    with pytest.raises(ValueError, match="instance 0 is behind the camera"):              # 2.2 away, but beside the camera
        scene.trace_scene(gen, [z], [SR.shifted("centre", 2.1, 0, -cam_dist + 0.5)])
    with pytest.raises(ValueError, match=r"2\^31"):
        scene.trace_scene(gen, torch.zeros(1024, 64), centre[None].expand(1024, 4, 4), window=1449)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="window"):
            scene.trace_scene(gen, [z], [centre], window=bad)
    with pytest.raises(ValueError, match="max_steps"):
        scene.trace_scene(gen, [z], [centre], max_steps=0)
    with pytest.raises(TypeError, match="unknown arguments"):
        scene.trace_scene(gen, [z], [centre], shadow_samples=4)
    with pytest.raises(ValueError, match="bias"):
        scene.trace_scene(gen, [z], [centre], bias=-1.0)
    for bad in (0, 1025, 1.5, True):
        with pytest.raises(ValueError, match="K="):
            scene.sample_scene(gen, bad, 0)
    with pytest.raises(ValueError, match="seed"):
        scene.sample_scene(gen, 3, -1)
    assert lib.TRACE_BATCH_MAX_ELEMS == SR.MAX_ELEMS


def test_sample_scene_is_reproducible_by_seed():
    from oi_amd import scene
    gen = fake_gen()
    before = np.random.get_state()[1].copy()
    zs, b2ws = scene.sample_scene(gen, 5, 7)
    assert np.array_equal(np.random.get_state()[1], before)          # the global generator is left as it was
    zs2, b2ws2 = scene.sample_scene(gen, 5, 7)
    zs3, b2ws3 = scene.sample_scene(gen, 5, 8)
    assert zs.shape == (5, 64) and b2ws.shape == (5, 4, 4) and b2ws.dtype == torch.float32
    assert torch.equal(zs, zs2) and torch.equal(b2ws, b2ws2)
    assert not torch.equal(zs, zs3) and not torch.equal(b2ws, b2ws3)
    rot = b2ws[:, :3, :3].double()
    assert float((rot @ rot.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6      # rigid poses
    np.random.seed(7)
    assert np.array_equal(np.asarray(gen.pose_prior(5), dtype=np.float32), b2ws.numpy())     # the pose prior's own draw
    scene.scene_windows(gen, b2ws)                                    # the prior's poses are in front of the camera


@pytest.mark.parametrize("R", [16, 24])
def test_default_window_holds_every_unit_sphere(R):
    """Brute force in float64 over an image extended far beyond S x S: no scene pixel whose ray passes within 1 of a box
    origin lies outside that instance's window, and the window is at most two pixels larger than the largest box."""
    from oi_amd import scene
    gen = fake_gen(R)
    poses = [p for kind in ("pair", "triple", "offscreen", "single") for _, p in SR.scene_poses(kind)]
    poses += list(scene.sample_scene(gen, 6, 3)[1])
    W, origin = scene.scene_windows(gen, torch.stack(poses))
    boxes = SR.min_window(poses, R)
    need = 0
    for (xlo, xhi, ylo, yhi), (x0, y0) in zip(boxes, origin):
        assert x0 <= xlo and xhi <= x0 + W - 1 and y0 <= ylo and yhi <= y0 + W - 1
        need = max(need, xhi - xlo + 1, yhi - ylo + 1)
    print(f"R={R}: default window {W}, largest bounding box {need}")
    assert need <= W <= need + 2
    # a caller's window keeps the projection centred
    W9, origin9 = scene.scene_windows(gen, torch.stack(poses), window=9)
    for (xlo, xhi, ylo, yhi), (x0, y0) in zip(boxes, origin9):
        assert W9 == 9 and abs((x0 + 4) - (xlo + xhi) / 2) <= 1.5 and abs((y0 + 4) - (ylo + yhi) / 2) <= 1.5


def test_restatement_is_self_consistent():
    rs = np.random.RandomState(0)
    E, W, S = 3, 5, 9
    origins = np.array([[1, 1], [3, 2], [-2, 6]])
    status = rs.choice([SR.MISS, SR.HIT, T.LIMIT], size=(E, W * W), p=[0.3, 0.6, 0.1])
    t = rs.rand(E, W * W).astype(np.float32)
    t[1] = np.where(rs.rand(W * W) < 0.5, 0.25, t[1])            # ties on purpose
    t[0] = np.where(rs.rand(W * W) < 0.5, 0.25, t[0])
    owner, owner_ray = SR.resolve(status, t, origins, W, S)
    # against a per-pixel loop
    for q in range(S * S):
        Y, X = divmod(q, S)
        cand = []
        for e in range(E):
            i, j = X - origins[e, 0], Y - origins[e, 1]
            if 0 <= i < W and 0 <= j < W and status[e, j * W + i] == SR.HIT:
                cand.append((t[e, j * W + i], e, j * W + i))
        if cand:
            best = min(cand)                                      # (t, e): equal t -> the lowest element index
            assert (owner[q], owner_ray[q]) == (best[1], best[2])
        else:
            assert owner[q] == owner_ray[q] == -1
    assert ((owner == 0) & (t[0][np.maximum(owner_ray, 0)] == 0.25)).any()                 # a tie was decided
    # one instance entered twice: element 0 owns every pixel
    o2, r2 = SR.resolve(np.stack([status[0]] * 2), np.stack([t[0]] * 2), np.stack([origins[0]] * 2), W, S)
    assert set(np.unique(o2)) <= {-1, 0} and (o2 == 0).sum() == (status[0] == SR.HIT).sum()
    sets = SR.visible_sets(owner, owner_ray, E)
    counts = [len(s) for s in sets]
    assert sum(counts) == (owner >= 0).sum() and all(len(np.unique(s)) == len(s) for s in sets)
    off = SR.offsets(counts)
    assert off.tolist() == [0, counts[0], counts[0] + counts[1]]
    # the visibility combination against a per-pixel loop
    n_vis, L = sum(counts), 2
    vis_slot = np.full((E, W * W), -1)
    for e in range(E):
        vis_slot[e, sets[e]] = rs.permutation(counts[e])
    shadow = rs.choice([SR.MISS, SR.HIT, SR.BACKFACING, T.LIMIT], size=(E, L, n_vis), p=[0.7, 0.1, 0.1, 0.1])
    vis = SR.combine_visibility(shadow, owner, owner_ray, vis_slot, off)
    for q in range(S * S):
        for l in range(L):
            if owner[q] < 0:
                assert vis[l, q] == 1
            else:
                g = off[owner[q]] + vis_slot[owner[q], owner_ray[q]]
                assert vis[l, q] == float(all(shadow[e, l, g] == SR.MISS for e in range(E)))
    assert 0 < vis[:, owner >= 0].mean() < 1
    # cull: the chord against a direct solve of |o + t d| = 1
    o = np.array([0.0, 0.0, -3.0])
    d = rs.randn(200, 3) * 0.2 + np.array([0, 0, 1.0])
    ent, near, far, c2 = SR.cull(o, d)
    assert ent.any() and (~ent).any()
    for k in np.nonzero(ent)[0]:
        for tt in (near[k], far[k]):
            assert abs(np.linalg.norm(o + tt * d[k]) - 1) < 1e-12
    inside = SR.cull(np.array([0.2, 0.0, 0.0]), np.array([1.0, 0, 0]))
    assert inside[0] and inside[1] == 0 and abs(inside[2] - 0.8) < 1e-15                     # origin inside: near clamps to 0
    assert not SR.cull(np.array([0, 0, 3.0]), np.array([0, 0, 1.0]))[0]                      # the sphere wholly behind
    # world transform and its bar
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = T.pose("centre").double().numpy()[:3, :3], [0.3, -5.8, 1.0]
    p = rs.randn(50, 3)
    w32 = (p.astype(np.float32) @ m[:3, :3].astype(np.float32).T + m[:3, 3].astype(np.float32)).astype(np.float64)
    exact = SR.transform(m.astype(np.float32), p.astype(np.float32))
    assert (np.abs(w32 - exact) <= SR.transform_bar(m, p)).all()


@pytest.mark.parametrize("kind", ["pair", "triple", "twice", "offscreen", "single", "nothing"])
def test_no_test_ray_lies_on_the_culls_edge(kind):
    """The GPU test lets the entered set differ from the restatement's only where |c2 - 1| <= 4 * 2^-24 (|o|^2 + 1); for the
    chosen poses no ray is that close, at any window the tests use."""
    from oi_amd import scene
    gen = fake_gen()
    S, K, K_inv, c2w, w2c = SR.camera(R_SCENE)
    poses = torch.stack([p for _, p in SR.scene_poses(kind)])
    for W in (9, 12, 16, None):
        Wn, origin = scene.scene_windows(gen, poses, W)
        for e, m in enumerate(poses):
            o, d = SR.scene_rays(SR.rigid_inverse(m.double().numpy()) @ c2w, K_inv, S)
            X, Y = SR.window_pixels(origin[e], Wn)
            ok = (X >= 0) & (X < S) & (Y >= 0) & (Y < S)
            ent, near, far, c2 = SR.cull(o, d[Y[ok], X[ok]])
            assert int((np.abs(c2 - 1) <= 4 * 2.0 ** -24 * (o @ o + 1)).sum()) == 0
            if kind in ("offscreen", "nothing") and abs(float(m[0, 3])) + abs(float(m[1, 3])) > 30:
                assert not ok.any()                                # wholly off screen: no ray at all


def test_analytic_scene_conditions():
    """The placement of the two-sphere scene keeps the float64 closed form ALONE within the caps the GPU test asserts: at
    most 3 % of the owned pixels and of the visible points excluded; the windows hold the spheres; both spheres own pixels,
    sphere 1 hides part of sphere 0; some points of sphere 0 are shadowed by sphere 1 that are lit without it; wherever both
    spheres are hit and the pixel is not excluded, the depths differ by more than the sum of the two depth bars (so the owner
    is decided); no visible point of sphere 0 has |n . l| below 1e-3."""
    sc = SR.analytic_scene()
    cf = SR.analytic_closed_form(sc)
    S, W = sc["S"], sc["W"]
    owned = cf["owner"] >= 0
    n_excl = int((cf["excluded"] & owned).sum())
    print("analytic scene: owned", int(owned.sum()), "by sphere", [int((cf["owner"] == e).sum()) for e in (0, 1)], "excluded", n_excl,
          "sphere-0 points", int(cf["on0"].sum()), "lit", int(cf["lit"].sum()), "lit alone", int(cf["lit_alone"].sum()),
          "shadow excluded", int(cf["shadow_excluded"].sum()), "worst depth bar", float(cf["bar"][owned & ~cf["excluded"]].max()))
    assert n_excl <= SR.AN_CAP * owned.sum()
    assert int(cf["shadow_excluded"].sum()) <= SR.AN_CAP * cf["on0"].sum()
    assert (cf["owner"] == 0).sum() > 40 and (cf["owner"] == 1).sum() > 40
    for e in range(2):                                            # every pixel a sphere is hit at lies in its window
        q = np.nonzero(np.isfinite(cf["depth"]) & (cf["owner"] == e))[0]
        X, Y = q % S, q // S
        x0, y0 = sc["origins"][e]
        assert (X >= x0).all() and (X < x0 + W).all() and (Y >= y0).all() and (Y < y0 + W).all()
    hidden = np.isfinite(cf["gap"]) & (cf["owner"] == 1)
    assert hidden.sum() > 5                                       # sphere 1 stands partly in front of sphere 0
    decided = np.isfinite(cf["gap"]) & ~cf["excluded"]
    assert (cf["gap"][decided] > cf["both_bar"][decided]).all()
    by_other = cf["lit_alone"] & ~cf["lit"]
    assert by_other.sum() > 5 and cf["lit"].sum() > 5
    assert np.abs(cf["ndl"]).min() > 1e-3
    assert float(cf["bar"][owned & ~cf["excluded"]].max()) < 3e-4


def golden_pair_oracle(o, d, near, far, entered, origins, W, S):
    """The fp64 oracle tracer on the entered rays of the 'pair' scene (rays (2, N, 3), float64).  -> status, t (2, N), the
    restatement's owner, owner_ray, and per pixel the gap between the two nearest oracle depths (inf with fewer than two)."""
    status, t = np.full(near.shape, SR.MISS, dtype=np.uint8), np.zeros(near.shape)
    for e, (seed, _) in enumerate(SR.scene_poses("pair")):
        idx = np.nonzero(entered[e])[0]
        te, se, _, _ = T.trace(T.Field(seed).sdf, o[e, idx], d[e, idx], near[e, idx], far[e, idx])
        status[e, idx], t[e, idx] = se, te
    owner, owner_ray = SR.resolve(status, t, origins, W, S)
    depth = np.full((2, S * S), np.inf)
    for e in range(2):
        X, Y = SR.window_pixels(origins[e], W)
        ok = (X >= 0) & (X < S) & (Y >= 0) & (Y < S) & (status[e] == SR.HIT)
        depth[e, (Y * S + X)[ok]] = t[e, ok]
    both = np.isfinite(depth).all(0)
    gap = np.where(both, np.abs(np.where(both, depth[0], 0.0) - np.where(both, depth[1], 0.0)), np.inf)
    return status, t, owner, owner_ray, gap


def test_golden_pair_conditions_on_the_oracle():
    """The golden two-instance scene on the oracle alone (float64 rays of the restatement): both instances own pixels, the
    nearer one hides part of the other, and at most 3 % of the owned pixels have their two nearest depths within 1e-4."""
    from oi_amd import scene
    gen = fake_gen()
    S, K, K_inv, c2w, w2c = SR.camera(R_SCENE)
    poses = torch.stack([p for _, p in SR.scene_poses("pair")])
    W, origins = scene.scene_windows(gen, poses, GOLDEN_W)
    N = W * W
    o, d, near, far, ent = np.zeros((2, N, 3)), np.zeros((2, N, 3)), np.zeros((2, N)), np.zeros((2, N)), np.zeros((2, N), dtype=bool)
    for e, m in enumerate(poses):
        oe, de = SR.scene_rays(SR.rigid_inverse(m.double().numpy()) @ c2w, K_inv, S)
        X, Y = SR.window_pixels(origins[e], W)
        ok = (X >= 0) & (X < S) & (Y >= 0) & (Y < S)
        o[e], d[e, ok] = oe, de[Y[ok], X[ok]]
        en, ne, fa, _ = SR.cull(oe, d[e, ok])
        ent[e, ok], near[e, ok], far[e, ok] = en, ne, fa
    status, t, owner, owner_ray, gap = golden_pair_oracle(o, d, near, far, ent, origins, W, S)
    owned = owner >= 0
    close = owned & (gap <= ORACLE_DEPTH_GAP)
    print("golden pair on the oracle: entered", ent.sum(1), "hits", (status == SR.HIT).sum(1), "owned", [int((owner == e).sum()) for e in (0, 1)],
          "both hit", int(np.isfinite(gap).sum()), "gap <= 1e-4", int(close.sum()), "smallest gap", float(gap.min()))
    assert (owner == 0).sum() > 20 and (owner == 1).sum() > 20
    assert np.isfinite(gap).sum() > 5 and (np.isfinite(gap) & (owner == 1)).sum() > 5
    assert close.sum() <= ORACLE_CAP * owned.sum()
    # the light of the GPU test's mutual-shadow check (from instance 0 towards instance 1): on the oracle some visible points of
    # instance 0 that face it have instance 1 in the way
    m0, m1 = (p.double().numpy() for p in poses)
    light = m1[:3, 3] - m0[:3, 3]
    r0 = owner_ray[owner == 0]
    pts = o[0, r0] + t[0, r0, None] * d[0, r0]
    _, g, _ = T.Field(0).full(pts)
    so, _, facing = T.shadow_rays(pts, g, T.light_object_dir(light, SR.rigid_inverse(m0)))
    world = SR.transform(m0, so[facing])
    o1 = SR.transform(SR.rigid_inverse(m1), world)
    d1 = np.broadcast_to(T.light_object_dir(light, SR.rigid_inverse(m1)), o1.shape)
    ent, near1, far1, _ = SR.cull(o1, d1)
    _, st1, _, _ = T.trace(T.Field(1).sdf, o1[ent], d1[ent], near1[ent], far1[ent])
    print("points of instance 0 facing the light", int(facing.sum()), "entering instance 1's sphere", int(ent.sum()), "blocked by it",
          int((st1 == SR.HIT).sum()))
    assert (st1 == SR.HIT).sum() > 3
