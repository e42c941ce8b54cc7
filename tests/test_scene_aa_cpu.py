"""CPU-only checks of the anti-aliasing of scenes (include/oi_scene_aa.h; oi_amd.scene): header <=> library
<=> binding for the three new symbols, the self-consistency of the restatement the GPU tests compare against
(tests/helpers/scene_aa_ref.py), the sub-pixel rays and the virtual image's size, the host layer's refusals -- and the
REHEARSAL of the conditions the GPU tests assert, on the float64 closed form of the analytic two-sphere scene and on the fp64
oracle tracer alone: the exclusions stay within scene_ref's 3 % cap at every sample count, and the classifier flags a share
of the golden two-instance scene that leaves the adaptive path something to save.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import test_scene_cpu as C
from conftest import ROOT
from helpers import aa_ref as AR
from helpers import cabi
from helpers import scene_aa_ref as SAR
from helpers import scene_ref as SR
from helpers import trace_ref as T

ENTRIES = ["oi_aa_resolve_strided", "oi_scene_aa_begin", "oi_scene_aa_classify"]
GOLDEN_FLAGGED_CAP = 0.25       # share of the scene pixels the defaults may flag on the golden pair (measured on the oracle: see the test)


def test_header_library_and_binding_agree():
    lib, L = cabi.built_lib()
    names, mirrors = cabi.check_header("oi_scene_aa.h", lib)
    assert sorted(names) == ENTRIES == lib.symbols("oi_scene_aa.h") and mirrors == []
    for n in ENTRIES:
        assert hasattr(L, n)
    text = cabi.read("oi_scene_aa.h")
    assert "struct" not in text and '#include "oi_aa.h"' in text and '#include "oi_scene.h"' in text
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"scene_aa.hip"' in src and "include/oi_scene_aa.h" in src
    from oi_amd import ops
    for n in ("scene_aa_classify", "scene_aa_begin", "aa_resolve_strided"):
        assert callable(getattr(ops, n))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _one_instance(a):
    """A synthetic surface of aa_ref (H x W) as a scene of ONE instance in an S x S scene image, S = max(H, W): local ray r is
    pixel r of the H x W block, the rows below the block are not owned."""
    H, W = a["H"], a["W"]
    S = max(H, W)
    owner, owner_ray = np.full((S, S), -1, np.int64), np.full((S, S), -1, np.int64)
    owner[:H, :W] = 0
    owner_ray[:H, :W] = np.arange(H * W).reshape(H, W)
    vis_slot = a["hit_slot"].astype(np.int64)[None]                              # (1, N): local ray r -> its hit
    return owner.reshape(-1), owner_ray.reshape(-1), vis_slot, a["hit_points"][None], a["grad"][None], S


@pytest.mark.parametrize("name", AR.SYNTHETIC)
def test_one_instance_is_the_single_view_classifier(name):
    a, _ = AR.synthetic(name)
    owner, owner_ray, vis_slot, pts, grad, S = _one_instance(a)
    status, hit_slot = SAR.dense(owner, owner_ray, vis_slot, pts.shape[1])
    for kw in (dict(), dict(plane=0.1), dict(cos=0.9), dict(plane=0.0, cos=0.0)):
        ref = AR.classify(status, hit_slot, pts[0], grad[0], S, S, **kw)
        assert np.array_equal(SAR.classify(owner, owner_ray, vis_slot, pts, grad, S, **kw), ref)
        mask, inst, plane, normal = SAR.classify(owner, owner_ray, vis_slot, pts, grad, S, parts=True, **kw)
        m1, p1, n1 = AR.classify(status, hit_slot, pts[0], grad[0], S, S, parts=True, **kw)
        assert not inst.any() and np.array_equal(mask, m1) and np.array_equal(plane, p1) and np.array_equal(normal, n1)
    # inside the H x W block the flags are the synthetic case's own
    img = SAR.classify(owner, owner_ray, vis_slot, pts, grad, S).reshape(S, S)[:a["H"] - 1, :a["W"]]
    assert np.array_equal(img, AR.classify(**a).reshape(a["H"], a["W"])[:a["H"] - 1])


def _patches(split_owner):
    """Two coplanar patches (the tilted plane of aa_ref) left and right of x = 3.5 in an 8 x 8 image, every pixel owned."""
    S = 8
    n = np.array([0.3, 0.0, 1.0]) / np.linalg.norm([0.3, 0.0, 1.0])
    ys, xs = np.mgrid[0:S, 0:S]
    pts = np.stack([xs * 0.05, ys * 0.05, -n[0] / n[2] * xs * 0.05], -1).reshape(-1, 3).astype(np.float32)
    grad = np.broadcast_to(n * 1.7, (S * S, 3)).astype(np.float32)
    left = (xs < S // 2).reshape(-1)
    owner = np.where(left | (not split_owner), 0, 1)
    # element e's window is the whole image; its visible hits are listed in a shuffled order
    E = 2
    vis_slot = np.full((E, S * S), -1, np.int64)
    points, grads = np.zeros((E, S * S, 3), np.float32), np.zeros((E, S * S, 3), np.float32)
    for e in range(E):
        mine = np.nonzero(owner == e)[0]
        perm = np.random.RandomState(e).permutation(len(mine))
        vis_slot[e, mine[perm]] = np.arange(len(mine))
        points[e, :len(mine)], grads[e, :len(mine)] = pts[mine[perm]], grad[mine[perm]]
    n_pad = int(max((owner == e).sum() for e in range(E)))
    return owner, np.arange(S * S), vis_slot, points[:, :n_pad], grads[:, :n_pad], S


def test_two_owners_flag_the_border_and_one_owner_nothing():
    owner, owner_ray, vis_slot, pts, grad, S = _patches(True)
    mask, inst, plane, normal = SAR.classify(owner, owner_ray, vis_slot, pts, grad, S, parts=True)
    assert not mask.any() and not plane.any() and not normal.any()
    img = inst.reshape(S, S)
    assert np.array_equal(np.nonzero(img.any(0))[0], [3, 4]) and np.array_equal(img.all(0), img.any(0))
    assert np.array_equal(SAR.classify(owner, owner_ray, vis_slot, pts, grad, S), inst)
    owner, owner_ray, vis_slot, pts, grad, S = _patches(False)
    assert not SAR.classify(owner, owner_ray, vis_slot, pts, grad, S).any()


def test_grazing_step_between_two_owners_is_flagged_on_both_sides():
    a, expected = AR.synthetic("grazing_step")
    owner, owner_ray, vis_slot, pts, grad, S = _one_instance(a)
    H, W = a["H"], a["W"]
    right = (np.arange(S * S) % S >= W // 2) & (owner >= 0)
    owner2 = np.where(right, 1, owner)
    # instance 1 holds the same hits under the same local rays: vis_slot, points and gradients repeated
    vis2, pts2, grad2 = np.repeat(vis_slot, 2, 0), np.repeat(pts, 2, 0), np.repeat(grad, 2, 0)
    mask, inst, plane, normal = SAR.classify(owner2, owner_ray, vis2, pts2, grad2, S, parts=True)
    img = inst.reshape(S, S)[:H - 1, :W]
    assert tuple(np.nonzero(img.any(0))[0].tolist()) == tuple(expected) and img.all(0)[list(expected)].all()
    # the plane test no longer speaks across the border (two frames), and one owner's side alone is a plane or a wall
    assert not plane.reshape(S, S)[:H - 1, :W].any()
    assert np.array_equal(SAR.classify(owner2, owner_ray, vis2, pts2, grad2, S).reshape(S, S)[:H - 1, :W],
                          AR.classify(**a).reshape(H, W)[:H - 1])


def test_out_of_range_entries_read_as_not_owned():
    owner, owner_ray, vis_slot, pts, grad, S = _patches(True)
    bad_owner = owner.copy()
    bad_owner[0], bad_owner[1] = 2, -7                                           # E = 2
    bad_ray = owner_ray.copy()
    bad_ray[2] = S * S
    bad_slot = vis_slot.copy()
    bad_slot[0, 3] = pts.shape[1]
    ok, _, _ = SAR.owned_rows(bad_owner, bad_ray, bad_slot, pts.shape[1])
    assert not ok[:4].any() and ok[4:].all()
    assert SAR.classify(bad_owner, bad_ray, bad_slot, pts, grad, S, parts=True)[0].reshape(S, S)[:2, :5].all()


# ---------------------------------------------------------------------------------------------------------------------
# rays and size
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_offsets_give_the_scene_rays():
    sc = SR.analytic_scene()
    S, W = sc["S"], sc["W"]
    pixels = np.arange(S * S)
    o, d, cov, ent, near, far = SAR.sub_rays(sc["c2b"], sc["K_inv"], S, W, sc["origins"], pixels, np.zeros((3, 2)))
    assert d.shape == (2, 2 * S * S, 3)
    for e in range(2):
        oe, de = SR.scene_rays(sc["c2b"][e], sc["K_inv"], S)
        for j in range(2):
            assert np.abs(d[e, j * S * S:(j + 1) * S * S] - de.reshape(-1, 3)).max() < 1e-13 and np.abs(o[e] - oe).max() < 1e-13
        X, Y = pixels % S, pixels // S
        x0, y0 = sc["origins"][e]
        inside = (X >= x0) & (X < x0 + W) & (Y >= y0) & (Y < y0 + W)
        assert np.array_equal(cov[e, :S * S], inside)
        en, ne, fa, _ = SR.cull(oe, de.reshape(-1, 3))
        assert np.array_equal(ent[e, :S * S], en & inside) and np.array_equal(near[e, :S * S], np.where(inside, ne, 0.0))
        assert not near[e][~ent[e]].any() and not far[e][~ent[e]].any()
    # an offset moves the ray by that share of a pixel pitch
    o2, d2, *_ = SAR.sub_rays(sc["c2b"], sc["K_inv"], S, W, sc["origins"], pixels[:-1], np.array([[0, 0], [0.5, 0.0]]))
    o3, d3, *_ = SAR.sub_rays(sc["c2b"], sc["K_inv"], S, W, sc["origins"], pixels[1:], np.array([[0, 0], [-0.5, 0.0]]))
    same_row = (pixels[:-1] % S) != S - 1
    assert np.abs(d2[:, same_row] - d3[:, same_row]).max() < 1e-13


@pytest.mark.parametrize("n_sub", [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 7 * 1246, 63 * 99 * 99, 46340 ** 2, 46340 ** 2 + 1])
def test_virtual_image_size(n_sub):
    from oi_amd import lib, scene
    Q = SAR.virtual_size(n_sub)
    assert Q * Q >= n_sub > (Q - 1) * (Q - 1) and Q * Q - n_sub < 2 * Q + 1
    if Q <= lib.SCENE_MAX_RESOLUTION:
        assert scene.virtual_image_size(n_sub, 1) == Q


# ---------------------------------------------------------------------------------------------------------------------
# rehearsals
# ---------------------------------------------------------------------------------------------------------------------
def analytic_flagged(sc):
    """The mask and instance criteria on the closed form's owner map (the plane and normal criteria need the traced surface):
    -> the flagged scene pixels, ascending."""
    cf = SR.analytic_closed_form(sc)
    S = sc["S"]
    owner = cf["owner"].reshape(S, S)
    flag = np.zeros((S, S), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = slice(max(0, -dy), S - max(0, dy)), slice(max(0, -dx), S - max(0, dx))
            yq, xq = slice(max(0, dy), S - max(0, -dy)), slice(max(0, dx), S - max(0, -dx))
            flag[ys, xs] |= owner[ys, xs] != owner[yq, xq]
    return np.nonzero(flag.reshape(-1))[0], cf


@pytest.mark.parametrize("Sa", [2, 4, 8, 64])
def test_analytic_rehearsal(Sa):
    """The conditions tests/test_gpu_scene_aa.py asserts on the analytic scene, on the closed form alone: the excluded
    sub-samples stay within scene_ref's cap, on the flagged pixels and on every pixel."""
    sc = SR.analytic_scene()
    S = sc["S"]
    pixels, cf = analytic_flagged(sc)
    owned = cf["owner"] >= 0
    by = [int((cf["owner"][pixels] == e).sum()) for e in (0, 1)]
    for name, pix in (("flagged", pixels), ("every pixel", np.arange(S * S))):
        owner, excluded = SAR.analytic_sub(sc, pix, AR.r2_pattern(Sa))
        share = excluded.mean()
        print(f"analytic scene Sa={Sa} {name}: pixels {len(pix)} of {S * S} (owned {int(owned.sum())}, flagged and owned by sphere 0 / 1: "
              f"{by}), sub-samples {len(owner)}, owners {[int((owner == e).sum()) for e in (-1, 0, 1)]}, excluded {int(excluded.sum())} "
              f"({share:.4f})")
        assert share <= SR.AN_CAP
        assert (owner == 0).sum() > 0 and (owner == 1).sum() > 0 and (owner == -1).sum() > 0
    assert 0 < len(pixels) < S * S // 2
    # a zero offset is the centre: the closed form's own owner
    o0, _ = SAR.analytic_sub(sc, np.arange(S * S), np.zeros((2, 2)))
    assert np.array_equal(o0[~cf["excluded"]], cf["owner"][~cf["excluded"]])


def test_golden_pair_rehearsal():
    """The classifier on the golden two-instance scene traced by the fp64 oracle alone (the restatement's float64 rays, as
    tests/test_scene_cpu.py traces them): the share of flagged scene pixels, and which criterion flags them."""
    from oi_amd import scene
    gen = C.fake_gen()
    S, K, K_inv, c2w, w2c = SR.camera(C.R_SCENE)
    poses = torch.stack([p for _, p in SR.scene_poses("pair")])
    W, origins = scene.scene_windows(gen, poses, C.GOLDEN_W)
    N, E = W * W, 2
    o, d, near, far, ent = np.zeros((E, N, 3)), np.zeros((E, N, 3)), np.zeros((E, N)), np.zeros((E, N)), np.zeros((E, N), dtype=bool)
    for e, m in enumerate(poses):
        oe, de = SR.scene_rays(SR.rigid_inverse(m.double().numpy()) @ c2w, K_inv, S)
        X, Y = SR.window_pixels(origins[e], W)
        ok = (X >= 0) & (X < S) & (Y >= 0) & (Y < S)
        o[e], d[e, ok] = oe, de[Y[ok], X[ok]]
        en, ne, fa, _ = SR.cull(oe, d[e, ok])
        ent[e, ok], near[e, ok], far[e, ok] = en, ne, fa
    status, t, owner, owner_ray, gap = C.golden_pair_oracle(o, d, near, far, ent, origins, W, S)
    sets = SR.visible_sets(owner, owner_ray, E)
    n_pad = max(len(x) for x in sets)
    vis_slot = np.full((E, N), -1, np.int64)
    points, grads = np.zeros((E, n_pad, 3), np.float32), np.zeros((E, n_pad, 3), np.float32)
    for e, (seed, _) in enumerate(SR.scene_poses("pair")):
        r = sets[e]
        vis_slot[e, r] = np.arange(len(r))
        pts = o[e, r] + t[e, r, None] * d[e, r]
        _, g, _ = T.Field(seed).full(pts)
        points[e, :len(r)], grads[e, :len(r)] = pts, g
    mask, inst, plane, normal = SAR.classify(owner, owner_ray, vis_slot, points, grads, S, parts=True)
    flagged = mask | inst | plane | normal
    share = flagged.mean()
    owned = owner >= 0
    print(f"golden pair on the oracle: flagged {int(flagged.sum())} of {S * S} scene pixels ({share:.4f}; {flagged[owned].mean():.3f} of the "
          f"{int(owned.sum())} owned), mask {int(mask.sum())}, instance {int(inst.sum())} ({int((inst & ~mask).sum())} alone), plane only "
          f"{int((plane & ~mask & ~inst).sum())}, normal only {int((normal & ~mask & ~inst & ~plane).sum())}")
    assert inst.sum() > 0 and (inst & ~mask).sum() > 0                            # the contour between the instances, where both sides hit
    assert 0 < share <= GOLDEN_FLAGGED_CAP
    Q = SAR.virtual_size(7 * int(flagged.sum()))
    print(f"golden pair: aa_samples=8 -> {7 * int(flagged.sum())} sub-samples per instance, virtual image {Q} x {Q}, padding "
          f"{Q * Q - 7 * int(flagged.sum())} rays")


# ---------------------------------------------------------------------------------------------------------------------
# the host layer's refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_gpu():
    from oi_amd import inference, scene
    from oi_amd.relight import LocalLight
    ok = [[0.0, 0.0], [0.25, -0.25]]
    bad = [dict(aa_samples=0), dict(aa_samples=65), dict(aa_samples=2.0), dict(aa_samples=True), dict(aa_plane=1.0),
           dict(aa_plane=float("nan")), dict(aa_cos=1.0), dict(aa_cos=-1e-3), dict(aa_adaptive=1),
           dict(aa_samples=2, aa_pattern=[[0.1, 0.0], [0.2, 0.2]]), dict(aa_samples=2, aa_pattern=[[0.0, 0.0], [0.6, 0.0]]),
           dict(aa_samples=3, aa_pattern=ok), dict(aa_samples=1, aa_pattern=ok)]
    for kw in bad:                                                                # before the generator is touched: there is none
        with pytest.raises(ValueError, match="trace_scene"):
            scene.trace_scene(None, None, None, **kw)
        with pytest.raises(ValueError, match="render_scene"):
            scene.render_scene(None, None, None, **kw)
        with pytest.raises(ValueError, match="scene_light_walk"):
            inference.scene_light_walk(None, None, None, **kw)
        with pytest.raises(ValueError, match="scene_light_orbit"):
            inference.scene_light_orbit(None, None, None, LocalLight(position=(0.0, 0.0, 2.0)), **kw)
    # the environment paths do not take the keywords
    gen, z, centre = C.fake_gen(), torch.zeros(64), T.pose("centre")
    with pytest.raises(TypeError, match="aa_samples"):
        scene.render_scene_env(gen, [z], [centre], [], aa_samples=4)
    from oi_amd.envlight import EnvLight
    gen.eval, gen.renderer = (lambda: None), types.SimpleNamespace(pack=types.SimpleNamespace(check=lambda: None))
    with pytest.raises(TypeError, match="aa_samples"):
        inference.scene_env_walk(gen, [z], [centre], EnvLight(np.zeros((9, 3))), n_frames=2, aa_samples=4)


def test_capture_transfer_refuses_an_anti_aliased_scene():
    from oi_amd import scene, trace
    s = scene.SceneSurface.__new__(scene.SceneSurface)
    s.aa = trace._check_aa(4, True, 0.5, 0.5, None, "x")
    with pytest.raises(ValueError, match="aa_samples=4"):
        s.capture_transfer(16)


def test_virtual_image_overflow_is_refused_by_arithmetic():
    from oi_amd import lib, scene
    assert scene.virtual_image_size(63 * 99 * 99, 1024) == 786                    # the largest case of the test scenes: fine
    Q = 1449                                                                      # 1024 * 1449^2 >= 2^31 > 1024 * 1448^2
    assert scene.virtual_image_size(1448 * 1448, 1024) == 1448
    with pytest.raises(ValueError, match=rf"{1448 * 1448 + 1} sub-sample rays.*{Q} x {Q}.*{1024 * Q * Q}"):
        scene.virtual_image_size(1448 * 1448 + 1, 1024)
    with pytest.raises(ValueError, match=r"2\^31"):
        scene.virtual_image_size(46341 ** 2, 1)
    with pytest.raises(ValueError, match=str(lib.SCENE_MAX_RESOLUTION)):
        scene.virtual_image_size(lib.SCENE_MAX_RESOLUTION ** 2 + 1, 1)
