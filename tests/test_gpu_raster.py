"""The mesh rasteriser on the MI355X (include/oi_raster.h; oi_amd.raster.render_mesh; oi_amd.inference.mesh_frames /
mesh_fidelity; oi_amd.mesh.load_obj).  The reference of the three stages is the restatement of
tests/helpers/raster_ref.py (float64 and integers), given THE GPU'S OWN snapped corners where the question is coverage; the
yardstick of the whole asset is oi_amd.trace.render_surface, existing code.  What the reference alone gives for the
conditions below is rehearsed in tests/test_raster_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_trace as G
from conftest import record_margin
from helpers import mesh_attr_ref as A
from helpers import mesh_tex_ref as X
from helpers import raster_ref as RR
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

NEAR, SMALL_MAX = 1e-3, 16
EPS = RR.EPS32
ENTRIES = ("oi_raster_setup", "oi_raster_fill", "oi_raster_resolve")
OUTPUTS = (("rays_o", 3, torch.float32), ("rays_d", 3, torch.float32), ("t", 1, torch.float32), ("status", 1, torch.uint8),
           ("hit_slot", 1, torch.int32), ("hit_points", 3, torch.float32), ("grad", 3, torch.float32), ("rgb", 3, torch.float32),
           ("triangle", 1, torch.int32), ("barycentric", 3, torch.float32))

_p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from oi_amd import lib
    return lib, lib.load()


def _dev(a, dtype=torch.float32):
    return guarded_copy(torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda())


class Views:
    """E test cameras on the device: what the three entries are given."""

    def __init__(self, cams):
        self.cams, self.E, self.R = cams, len(cams), cams[0]["R"]
        stack = lambda k: _dev(np.stack([c[k] for c in cams]))
        self.c2b, self.b2c, self.offs = stack("c2b"), stack("b2c"), stack("offs")
        self.K, self.kinv = _dev(cams[0]["K"]), _dev(cams[0]["kinv"])


def cameras(R, E, seed=0):
    """E cameras that share their intrinsics (the entries take one K) and differ in pose and crop offsets."""
    cams = [RR.camera(R, seed + e) for e in range(E)]
    for c in cams[1:]:
        c["K"], c["kinv"] = cams[0]["K"], cams[0]["kinv"]
    return cams


def run_setup(v, pos, tris, small_max=SMALL_MAX, near=NEAR):
    lib, L = _lib()
    E, F, V = v.E, len(tris), len(pos)
    d_pos, d_tris = _dev(pos), _dev(tris, torch.int32)
    out = {"corners": guarded_empty((E, F, 3, 2), torch.int32, what="corners"), "bbox": guarded_empty((E, F, 4), torch.int32, what="bbox"),
           "cls": guarded_empty((E, F), torch.uint8, what="cls"),
           "small_list": guarded_empty((E, F), torch.int32, what="small_list", must_write=False),
           "large_list": guarded_empty((E, F), torch.int32, what="large_list", must_write=False),
           "counts": guarded_empty((E, 2), torch.int32, what="counts", must_write=F > 0)}
    rc = L.oi_raster_setup(_p(v.b2c), _p(v.K), _p(v.offs), v.R, E, _p(d_pos), _p(d_tris), V, F, near, small_max,
                           *(_p(out[k]) for k in ("corners", "bbox", "cls", "small_list", "large_list", "counts")), None)
    assert rc == 0, L.oi_last_error()
    torch.cuda.synchronize()
    out["pos"], out["tris"] = d_pos, d_tris
    return out


def run_fill(v, s):
    lib, L = _lib()
    E, N = v.E, v.R * v.R
    zbuf = guarded_empty((E, N), torch.int64, what="zbuf", must_write=False)
    zbuf.fill_(-1)
    rc = L.oi_raster_fill(_p(v.c2b), _p(v.kinv), _p(v.offs), v.R, E, _p(s["pos"]), _p(s["tris"]), len(s["pos"]), len(s["tris"]),
                          *(_p(s[k]) for k in ("corners", "bbox", "small_list", "large_list", "counts")), _p(zbuf), None)
    assert rc == 0, L.oi_last_error()
    torch.cuda.synchronize()
    return zbuf


def run_resolve(v, s, zbuf, vertex=None, texture=None, want=tuple(n for n, _, _ in OUTPUTS), plain=False):
    """-> {name: tensor}: guarded outputs (plain: ordinary tensors pre-filled with a pattern, for the 1024 combinations)."""
    lib, L = _lib()
    E, N = v.E, v.R * v.R
    out = {}
    for name, c, dt in OUTPUTS:
        if name in want:
            shape = (E, N) if c == 1 else (E, N, 3)
            out[name] = torch.full(shape, 77, dtype=dt, device="cuda") if plain else guarded_empty(shape, dt, what=name)
    src = [None, None, None, 0, 0, None, None, None, None]
    if vertex is not None:
        src[0], src[1], mode = _p(vertex[0]), _p(vertex[1]), lib.RASTER_VERTEX
    else:
        uv, am, nm = texture
        src[2], src[3], src[4], mode = _p(uv), am.shape[1], am.shape[0], lib.RASTER_TEXTURE
        src[5 if am.dtype == torch.uint8 else 6] = _p(am)
        src[7 if nm.dtype == torch.uint8 else 8] = _p(nm)
    rc = L.oi_raster_resolve(_p(v.c2b), _p(v.kinv), _p(v.offs), v.R, E, _p(s["pos"]), _p(s["tris"]), len(s["pos"]), len(s["tris"]),
                             _p(zbuf), mode, *src, *(_p(out.get(n)) for n, _, _ in OUTPUTS), None)
    assert rc == 0, L.oi_last_error()
    torch.cuda.synchronize()
    return out


def keys_of(zbuf, R):
    """zbuf (E, N) int64 -> ids (E, R, R) int64 (-1 where empty) and the key's depth (E, R, R) float32 (NaN where empty)."""
    z = zbuf.cpu().numpy().astype(np.int64)
    empty = z == -1
    ids = np.where(empty, -1, z & 0xffffffff).reshape(-1, R, R)
    t = ((z >> 32) & 0xffffffff).astype(np.uint32).view(np.float32)
    return ids, np.where(empty, np.nan, t).reshape(-1, R, R)


def gpu_reference(cam, pos, tris, s, e):
    """RR.raster from the GPU's own corners, classes and boxes of view e."""
    return RR.raster(cam, pos, tris, s["corners"][e].cpu().numpy().astype(np.int64), s["cls"][e].cpu().numpy(),
                     s["bbox"][e].cpu().numpy().astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# setup
# ---------------------------------------------------------------------------------------------------------------------
def check_setup(v, pos, tris, s, small_max):
    F = len(tris)
    for e, cam in enumerate(v.cams):
        _, fixed, rcls, _ = RR.setup(cam, pos, tris, NEAR, small_max)
        cls = s["cls"][e].cpu().numpy()
        corners = s["corners"][e].cpu().numpy().astype(np.int64)
        kept = cls != RR.DROPPED
        assert np.array_equal(kept, rcls != RR.DROPPED)
        # snapped corners within one unit of the float64 projection: half a unit is the snap's; the fp32 projection adds a
        # few eps of the coordinate, times the condition of the division by the camera depth (the terms of pc_z over pc_z)
        # for a vertex close to the camera plane, whose coordinate is far off the screen; zeros where dropped
        _, depth = RR.project(cam, pos)
        cond = (np.abs(pos.astype(np.float64)) @ np.abs(cam["b2c"][2, :3]) + abs(cam["b2c"][2, 3])) / np.abs(depth)
        bar = 1.0 + 16 * EPS * np.abs(fixed) * (1.0 + cond[tris])[..., None]
        assert F == 0 or not kept.any() or (np.abs(corners[kept] - fixed[kept]) <= bar[kept]).all()
        on_screen = kept & (np.abs(fixed) < 64 * v.R * RR.FIX).all((1, 2)) if F else kept
        assert not on_screen.any() or np.abs(corners[on_screen] - fixed[on_screen]).max() <= 1.0
        assert (corners[~kept] == 0).all()
        # classes and boxes are exact given the GPU's own corners
        ecls, ebox = RR.classify(corners, kept, v.R, small_max)
        assert np.array_equal(cls, ecls) and np.array_equal(s["bbox"][e].cpu().numpy(), ebox)
        if F:
            ns, nl = s["counts"][e].tolist()
            assert (ns, nl) == (int((cls == RR.SMALL).sum()), int((cls == RR.LARGE).sum()))
            assert sorted(s["small_list"][e, :ns].tolist()) == np.nonzero(cls == RR.SMALL)[0].tolist()
            assert sorted(s["large_list"][e, :nl].tolist()) == np.nonzero(cls == RR.LARGE)[0].tolist()


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("F", [0, 1, 3, 65, 257])
@pytest.mark.parametrize("R", [1, 2, 7, 33])
def test_setup(R, F, E):
    """Random triangles of every size about the unit ball (some reach behind the camera at 2.5: dropped), one workgroup and
    more than one, ragged."""
    rs = np.random.RandomState(1000 * R + 10 * F + E)
    pos = np.concatenate([RR.soup(F, F + R, size=0.5)[0], (rs.rand(F, 3) * 7 - 3.5).astype(np.float32)]) if F else np.zeros((1, 3), np.float32)
    tris = RR.soup(F, 0)[1].copy() if F else np.zeros((0, 3), np.int32)
    if F:
        tris[::4, 2] = 3 * F + np.arange(len(tris[::4]))      # every fourth triangle reaches to a far, random vertex
    v = Views(cameras(R, E, seed=R))
    s = run_setup(v, pos, tris)
    if F == 0:     # nothing is launched: the counters keep their poison
        assert bool((s["counts"] == 0x7F8B0D1E).all())
        return
    check_setup(v, pos, tris, s, SMALL_MAX)


def unproject(cam, X_, Y_, depth):
    """The box-frame point at camera depth `depth` that projects onto the raster coordinate (X_, Y_)."""
    R = cam["R"]
    scale = R / (R - 1) if R > 1 else 1.0
    pc = np.linalg.inv(cam["K"]) @ np.array([X_ * scale + cam["offs"][0], Y_ * scale + cam["offs"][1], 1.0]) * depth
    return (cam["c2b"][:3, :3] @ pc + cam["c2b"][:3, 3]).astype(np.float32)


@pytest.mark.parametrize("small_max", [16, 19, 20])
def test_setup_classes(small_max):
    """One triangle per rule, placed through the camera's inverse so that its corners snap where the rule is decided."""
    R = 7
    cam = RR.camera(R, 4)
    u = lambda *c: [unproject(cam, x, y, d) for x, y, d in c]
    named = [("behind near", u((1, 1, 2.0), (3, 1, 2.0), (2, 3, 0.5 * NEAR)), RR.DROPPED),
             ("behind the camera", u((1, 1, 2.0), (3, 1, 2.0), (2, 3, -1.0)), RR.DROPPED),
             ("zero area", u((1, 1, 2.0), (2, 2, 2.0), (3, 3, 2.0)), RR.EMPTY),
             ("off the screen", u((-5, 1, 2.0), (-3, 1, 2.0), (-4, 3, 2.0)), RR.EMPTY),
             ("between the centres", u((1.1, 1.1, 2.0), (1.8, 1.2, 2.0), (1.4, 1.85, 2.0)), RR.EMPTY),
             ("larger than the screen", u((-20, -20, 2.0), (40, -20, 2.0), (-20, 40, 2.0)), RR.LARGE),
             ("a box of 16 centres", u((0, 0, 2.0), (3, 0, 2.0), (0, 3, 2.0)), RR.SMALL if small_max >= 16 else RR.LARGE),
             ("a box of 20 centres", u((0, 0, 2.0), (4, 0, 2.0), (0, 3, 2.0)), RR.SMALL if small_max >= 20 else RR.LARGE),
             ("beyond the coordinate limit", u((1, 1, 2.0), (3, 1, 2.0), (5.0e6, 3, 2.0)), RR.DROPPED)]
    pos = np.concatenate([np.stack(c) for _, c, _ in named]).astype(np.float32)
    tris = np.arange(3 * len(named), dtype=np.int32).reshape(-1, 3)
    v = Views([cam])
    s = run_setup(v, pos, tris, small_max)
    got = s["cls"][0].tolist()
    for (name, _, exp), g in zip(named, got):
        assert g == exp, (name, g, exp)
    check_setup(v, pos, tris, s, small_max)
    assert s["bbox"][0, 5].tolist() == [0, 0, R - 1, R - 1] and s["bbox"][0, 6].tolist() == [0, 0, 3, 3]
    # a bad index drops the triangle, nothing is read outside pos
    bad = tris.copy()
    bad[6, 1] = len(pos)
    assert run_setup(v, pos, bad, small_max)["cls"][0].tolist()[6] == RR.DROPPED


# ---------------------------------------------------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------------------------------------------------
def fill_case(name):
    if name == "sphere":
        return RR.sphere_case()
    if name == "soup":
        return RR.soup_case()
    cam = RR.camera(33, 2)
    pos, tris = RR.quad(flip=name == "quad_flipped")
    return cam, pos, tris


def check_fill(cam, pos, tris, s, zbuf, e=0, soup=False):
    """ids equal the reference wherever its two nearest candidates differ by more than the depth bar; the key's depth within
    the bar.  -> (ids, t, the reference tuple)."""
    R = cam["R"]
    ids, t = keys_of(zbuf, R)
    ids, t = ids[e], t[e]
    rids, rt, second, cosine, count = gpu_reference(cam, pos, tris, s, e)
    assert np.array_equal(ids >= 0, rids >= 0)
    left = RR.unexamined(rt, second, cosine)
    covered = int((rids >= 0).sum())
    assert covered > 50 and left.sum() <= 0.02 * covered
    assert np.array_equal(ids[~left], rids[~left])
    if left.any():   # within the bar either candidate may win; the depth still has to be the nearest one's
        assert (np.abs(t[left] - rt[left]) <= 3.0 * RR.depth_bar(rt[left], cosine[left])).all()
    on = (rids >= 0) & ~left & (cosine >= RR.GRAZING)
    err = np.abs(t[on].astype(np.float64) - rt[on]) / RR.depth_bar(rt[on], cosine[on])
    assert err.max() <= 1.0
    return ids, t, (rids, rt, second, cosine, count), float(err.max()), int(left.sum())


@pytest.mark.parametrize("name", ["sphere", "quad", "quad_flipped", "soup"])
def test_fill_is_the_integer_reference(name):
    cam, pos, tris = fill_case(name)
    v = Views([cam])
    s = run_setup(v, pos, tris)
    zbuf = run_fill(v, s)
    ids, t, ref, worst, left = check_fill(cam, pos, tris, s, zbuf)
    record_margin(f"raster_fill[{name}]", "depth_over_bar", worst)
    print(name, "covered", int((ids >= 0).sum()), "unexamined", left, "depth / bar", worst, "overlapped", int((ref[4] > 1).sum()))
    if name != "soup":
        assert left == 0        # sphere and quad: the ids are the reference's exactly
    if name == "soup":
        assert (ref[4] > 1).sum() > 100
    # the two paths, and a second run: identical bytes
    for small_max in (0, 1 << 30):
        s2 = run_setup(v, pos, tris, small_max)
        cls = s2["cls"][0]
        assert not bool((cls == (RR.SMALL if small_max == 0 else RR.LARGE)).any())
        assert torch.equal(run_fill(v, s2), zbuf)
    assert torch.equal(run_fill(v, s), zbuf)


def hand_fill(cam, corners, nearest_first, path):
    """oi_raster_fill on HAND-WRITTEN snapped corners, boxes, lists and counts (setup's outputs are fill's inputs): triangle
    f lies in a plane of its own in front of the camera, so every ray meets it at a finite t > 0, and the planes are stacked
    by `nearest_first` (True: triangle 0 nearest).  path: "small" or "large", the list that holds every triangle.
    -> ids (R, R)."""
    R, F = cam["R"], len(corners)
    cls, bbox = RR.classify(corners, np.ones(F, dtype=bool), R, SMALL_MAX)
    assert (cls >= RR.SMALL).all()
    depth = [2.0 + 0.05 * (f if nearest_first else F - 1 - f) for f in range(F)]
    pos = np.stack([unproject(cam, x, y, depth[f]) for f in range(F) for x, y in ((-30, -30), (60, -30), (-30, 60))])
    v = Views([cam])
    order = np.random.RandomState(F).permutation(F).astype(np.int32)        # the lists are in no fixed order
    fill = np.full(F, -7, dtype=np.int32)                                    # past the count: never read as a triangle
    s = {"corners": _dev(corners[None], torch.int32), "bbox": _dev(bbox[None], torch.int32),
         "small_list": _dev((order if path == "small" else fill)[None], torch.int32),
         "large_list": _dev((order if path == "large" else fill)[None], torch.int32),
         "counts": _dev(np.array([[F, 0] if path == "small" else [0, F]]), torch.int32),
         "pos": _dev(pos), "tris": _dev(np.arange(3 * F).reshape(F, 3), torch.int32)}
    ids, t = keys_of(run_fill(v, s), R)
    assert np.array_equal(np.isfinite(t[0]), ids[0] >= 0)
    return ids[0]


@pytest.mark.parametrize("path", ["small", "large"])
@pytest.mark.parametrize("nearest_first", [True, False])
@pytest.mark.parametrize("case", ["square", "square_flipped", "fan"])
def test_fill_top_left_rule_on_centres_that_lie_on_edges(case, nearest_first, path):
    """The kernel's tie rule itself: centres that lie EXACTLY on snapped edges.  The cases are those of
    tests/test_raster_cpu.py -- the 8 x 8 square whose shared diagonal runs through the centres (k, k), in both orientations
    of its second triangle, and the closed fan whose apex is the centre (6, 6).  The expected owner of every centre is
    covers_int's; the planes are stacked both ways, so a centre covered TWICE would go to the nearer, wrong triangle in one
    of the two runs, and a centre covered by NONE (a crack) is off the mesh in both."""
    cam = RR.camera(13, 8)
    corners = RR.tie_fan()[0] if case == "fan" else RR.tie_square(case == "square_flipped")
    want = RR.owners(corners, 13)
    ids = hand_fill(cam, corners, nearest_first, path)
    assert np.array_equal(ids, want)
    if case == "fan":
        assert ids[6, 6] >= 0 and (want >= 0).sum() > 80
        return
    for k in range(1, 8):
        assert ids[k, k] == want[k, k] >= 0                   # the shared diagonal: covered, by the owner
    assert (ids[1:8, 1:8] >= 0).all()                          # no crack inside
    assert (ids[0, 0:8] >= 0).all() and (ids[0:8, 0] >= 0).all()       # the top and the left outline are owned
    assert (ids[8, :] == -1).all() and (ids[:, 8] == -1).all()         # the bottom and the right outline are not
    assert (ids[9:, :] == -1).all() and (ids[:, 9:] == -1).all()


def test_fill_does_not_depend_on_the_triangle_order():
    cam, pos, tris = RR.sphere_case()
    v = Views([cam])
    s = run_setup(v, pos, tris)
    ids, t = keys_of(run_fill(v, s), cam["R"])
    perm = np.random.RandomState(0).permutation(len(tris))
    s2 = run_setup(v, pos, tris[perm])
    ids2, t2 = keys_of(run_fill(v, s2), cam["R"])
    assert np.array_equal(t.view(np.uint32), t2.view(np.uint32))                  # the same depth, bit for bit
    assert np.array_equal(np.where(ids2 >= 0, perm[np.maximum(ids2, 0)], -1), ids)    # new index k is old triangle perm[k]
    # a duplicated triangle: the lower index wins wherever the duplicate is visible
    dup = np.concatenate([tris, tris[::-1]])
    s3 = run_setup(v, pos, dup)
    ids3, t3 = keys_of(run_fill(v, s3), cam["R"])
    assert np.array_equal(t3.view(np.uint32), t.view(np.uint32))
    F = len(tris)
    assert np.array_equal(ids3, np.where(ids >= 0, np.minimum(ids, 2 * F - 1 - ids), -1))


def test_views_in_one_launch_are_the_single_launches():
    pos, tris = RR.icosphere(2, RR.SPHERE_RADIUS)
    cams = cameras(33, 3, seed=5)
    v = Views(cams)
    s = run_setup(v, pos, tris)
    zbuf = run_fill(v, s)
    vn = _dev(RR.unit(pos.astype(np.float64)))
    va = _dev(pos * 0.8 + 0.5)
    g = run_resolve(v, s, zbuf, vertex=(vn, va))
    for e, cam in enumerate(cams):
        v1 = Views([cam])
        s1 = run_setup(v1, pos, tris)
        for k in ("corners", "bbox", "cls"):
            assert torch.equal(s1[k][0], s[k][e])
        z1 = run_fill(v1, s1)
        assert torch.equal(z1[0], zbuf[e])
        g1 = run_resolve(v1, s1, z1, vertex=(vn, va))
        for k in g:
            assert torch.equal(g1[k][0].view(torch.uint8), g[k][e].view(torch.uint8)), k
        check_fill(cam, pos, tris, s, zbuf, e)


# ---------------------------------------------------------------------------------------------------------------------
# resolve
# ---------------------------------------------------------------------------------------------------------------------
# albedo = A p + b: within [0.1, 0.9] on the ball of radius 0.5 the meshes live in, the extrapolated gutter texels included
AFFINE = 0.65 * np.array([[0.5, -0.2, 0.1], [0.1, 0.6, -0.3], [-0.4, 0.2, 0.5]]), np.array([0.5, 0.45, 0.55])


def albedo_of(p):
    return np.asarray(p, dtype=np.float64) @ AFFINE[0].T + AFFINE[1]


def position_bar(cam, t, cosine, pts):
    """How far the fp32 hit point may lie from the float64 one: the depth bar along the ray, and the rounding of o + t d."""
    return RR.depth_bar(t, cosine) + 8.0 * EPS * (np.linalg.norm(pts, axis=-1) + np.abs(t))


def min_altitude(v):
    """The smallest altitude of the triangles v (n, 3, 3): a barycentric changes by at most |dp| / altitude."""
    area2 = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=-1)
    return area2 / max(np.linalg.norm(v[:, k] - v[:, (k + 1) % 3], axis=-1).max() for k in range(3))


def resolved_reference(cam, pos, tris, s, zbuf, g):
    """What every resolve test needs of one view: the pixels on the mesh off the grazing rim, their float64 depth, point,
    triangle rows and barycentrics, and the bars that follow from the position's."""
    R = cam["R"]
    ids, _ = keys_of(zbuf, R)
    ids = ids[0]
    o, d = RR.rays(cam)
    tri = g["triangle"][0].cpu().numpy().reshape(R, R)
    assert np.array_equal(tri, ids)
    on = ids >= 0
    v = pos.astype(np.float64)[tris[ids[on]]]
    t64, nd = np.zeros(on.sum()), np.zeros(on.sum())
    for k, (vv, dd) in enumerate(zip(v, d[on])):
        t64[k], nd[k] = RR.plane_t(vv, o, dd)
    cosine = np.abs(nd)
    keep = cosine >= RR.GRAZING
    assert (~keep).sum() <= 0.05 * on.sum()
    p64 = o + t64[:, None] * d[on]
    return {"on": on, "keep": keep, "t": t64, "cosine": cosine, "p": p64, "v": v, "rows": tris[ids[on]], "ids": ids[on],
            "bary": RR.barycentric(v, p64), "pbar": position_bar(cam, t64, cosine, p64), "alt": min_altitude(v), "o": o, "d": d}


def test_resolve_depth_rays_and_defined_values():
    cam, pos, tris = RR.sphere_case()
    v = Views([cam])
    s = run_setup(v, pos, tris)
    zbuf = run_fill(v, s)
    g = run_resolve(v, s, zbuf, vertex=(_dev(RR.unit(pos.astype(np.float64))), _dev(albedo_of(pos))))
    R, N = cam["R"], cam["R"] ** 2
    r = resolved_reference(cam, pos, tris, s, zbuf, g)
    on, keep = r["on"].reshape(-1), r["keep"]
    num = lambda k: g[k][0].cpu().numpy()
    # the rays are make_ray's (float64 restatement), everywhere
    assert np.abs(num("rays_o") - r["o"][None]).max() <= 4 * EPS * np.abs(r["o"]).max()
    assert np.abs(num("rays_d") - r["d"].reshape(N, 3)).max() <= 16 * EPS
    assert np.array_equal(num("hit_slot"), np.arange(N)) and np.array_equal(num("status"), on.astype(np.uint8))
    # the key's depth is the resolved depth, bit for bit (one device function)
    _, tk = keys_of(zbuf, R)
    t = num("t")
    assert np.array_equal(t[on].view(np.uint32), tk[0].reshape(-1)[on].view(np.uint32))
    err = np.abs(t[on].astype(np.float64) - r["t"])[keep] / RR.depth_bar(r["t"], r["cosine"])[keep]
    record_margin("raster_resolve[sphere]", "depth_over_bar", float(err.max()))
    assert err.max() <= 1.0
    assert (np.abs(num("hit_points")[on] - r["p"]).max(-1)[keep] <= r["pbar"][keep]).all()
    # against the analytic sphere: within the faces' sag (raster_ref.face_sag), radially and along the ray, plus the bar
    full = np.full((R, R), np.nan)
    full[r["on"]] = t[on]
    radial, along, ok = RR.sphere_gaps(cam, full, RR.SPHERE_RADIUS)
    sag = RR.face_sag(RR.SPHERE_RADIUS, RR.longest_edge(pos, tris))
    sel = r["on"].copy()
    sel[r["on"]] = keep
    bar = np.zeros((R, R))
    bar[r["on"]] = r["pbar"]
    assert (radial[sel] >= -bar[sel]).all() and (radial[sel] <= sag + bar[sel]).all()
    bound = RR.along_ray_bound(cam, RR.SPHERE_RADIUS, sag)
    assert (along[sel & ok] >= -bar[sel & ok]).all() and (along[sel & ok] <= bound[sel & ok] + bar[sel & ok]).all()
    record_margin("raster_resolve[sphere]", "radial_depth_over_sag", float(radial[sel].max() / sag))
    # off the mesh: the defined values
    off = ~on
    assert off.sum() > 100 and (t[off] == 0).all() and (num("triangle")[off] == -1).all()
    for k in ("hit_points", "grad", "rgb", "barycentric"):
        assert (num(k)[off] == 0).all(), k
    # barycentrics: non-negative, sum to one, the float64 ones within the position's bar over the altitude
    b = num("barycentric")[on]
    assert (b >= 0).all() and np.abs(b.sum(-1) - 1).max() <= 4 * EPS
    assert (np.abs(b - r["bary"]).max(-1)[keep] <= (2 * r["pbar"] / r["alt"] + 16 * EPS)[keep]).all()


@pytest.mark.parametrize("mode", ["vertex", "texture_f32", "texture_u8"])
def test_resolve_attributes(mode):
    """The albedo is an AFFINE function of position, which barycentric interpolation and the bilinear lookup of an atlas
    sampled at helpers/mesh_tex_ref.py's points both reproduce exactly: the resolved colour must be that function at the
    hit point -- through v = 1 - y / H, row 0 on top, the + 0.5 centres, both half cells and the gutter.  Bars: the
    gradient times the position's bar, a few fp32 eps of the lookup's arithmetic per texel of the atlas' side, and for byte
    atlases the quantisation, 2^-8.  The normal is held against the float64 restatement of the same lookup."""
    cam, pos, tris = RR.sphere_case()
    v = Views([cam])
    s = run_setup(v, pos, tris)
    zbuf = run_fill(v, s)
    F, Tx = len(tris), 5
    normals = RR.unit(pos.astype(np.float64))
    grad_a = np.abs(AFFINE[0]).sum(1).max()
    if mode == "vertex":
        vn, va = normals.astype(np.float32), albedo_of(pos).astype(np.float32)
        g = run_resolve(v, s, zbuf, vertex=(_dev(vn), _dev(va)))
    else:
        W, H, _, _ = X.layout(F, Tx)
        px = X.pixels(F, Tx)
        pts = X.points(pos, tris, Tx)
        am, nm = np.zeros((H, W, 3)), np.full((H, W, 3), 0.5)
        am[px[..., 1], px[..., 0]] = albedo_of(pts)
        nm[px[..., 1], px[..., 0]] = RR.unit(pts)
        uv = X.corner_uv(F, Tx).astype(np.float32)
        if mode == "texture_u8":
            am, nm = X.quant8(am), X.quant8(nm * 0.5 + 0.5)
            g = run_resolve(v, s, zbuf, texture=(_dev(uv), _dev(am, torch.uint8), _dev(nm, torch.uint8)))
        else:
            am, nm = am.astype(np.float32), nm.astype(np.float32)
            g = run_resolve(v, s, zbuf, texture=(_dev(uv), _dev(am), _dev(nm)))
    r = resolved_reference(cam, pos, tris, s, zbuf, g)
    on, keep = r["on"].reshape(-1), r["keep"]
    rgb, nn = g["rgb"][0].cpu().numpy()[on].astype(np.float64), g["grad"][0].cpu().numpy()[on].astype(np.float64)
    bary_bar = 2 * r["pbar"] / r["alt"] + 16 * EPS
    if mode == "vertex":
        en, _ = RR.vertex_attr(r["rows"], r["bary"], vn, va)
        a_bar = grad_a * r["pbar"] + 16 * EPS
        spread = max(np.abs(normals[tris[:, k]] - normals[tris[:, (k + 1) % 3]]).sum(-1).max() for k in range(3))
        n_bar = 2 * spread * bary_bar + 16 * EPS
    else:
        en, _ = RR.texture_attr(uv.astype(np.float64)[r["ids"]], r["bary"], am, nm, X.sample_bilinear)
        lookup = 16 * EPS * (W + H)                       # u W and (1 - v) H in fp32: a few eps of a coordinate up to W, H
        quant = 2.0 ** -8 if mode == "texture_u8" else 0.0
        a_bar = grad_a * r["pbar"] + lookup + quant
        # neighbouring texels of one triangle differ by at most `step`; a barycentric error moves the lookup by (T - 2) texels
        nmf = nm.astype(np.float64) / 255 * 2 - 1 if mode == "texture_u8" else nm.astype(np.float64)
        own = nmf[px[..., 1], px[..., 0]]
        step = np.abs(own[:, 1:] - own[:, :-1]).sum(-1).max()
        n_bar = 2 * step * ((Tx - 2) * bary_bar + lookup) + 16 * EPS
    ea = np.abs(rgb - albedo_of(r["p"])).max(-1)
    eb = np.abs(nn - en).max(-1)
    worst_a, worst_n = float((ea / a_bar)[keep].max()), float((eb / n_bar)[keep].max())
    record_margin(f"raster_attributes[{mode}]", "albedo_over_bar", worst_a)
    record_margin(f"raster_attributes[{mode}]", "normal_over_bar", worst_n)
    print(mode, "albedo", float(ea[keep].max()), "over bar", worst_a, "normal", float(eb[keep].max()), "over bar", worst_n)
    assert worst_a <= 1.0 and worst_n <= 1.0
    assert np.abs(np.linalg.norm(nn, axis=-1) - 1).max() <= 8 * EPS
    if mode != "vertex":   # and the normal map means what it says: the sphere's own normal at the hit point, to the facets' size
        assert np.abs(nn - RR.unit(r["p"]))[keep].max() < 0.05 + (2.0 ** -7 if mode == "texture_u8" else 0.0)


def test_resolve_every_combination_of_outputs():
    """All 1024 combinations write what the full launch writes (ordinary tensors pre-filled with a pattern); each output
    alone, all but each one, none and all of them also into guarded buffers."""
    cam = RR.camera(7, 6)
    pos, tris = RR.icosphere(1, RR.SPHERE_RADIUS)
    v = Views([cam])
    s = run_setup(v, pos, tris)
    zbuf = run_fill(v, s)
    src = (_dev(RR.unit(pos.astype(np.float64))), _dev(albedo_of(pos)))
    names = [n for n, _, _ in OUTPUTS]
    full = run_resolve(v, s, zbuf, vertex=src, plain=True)
    assert int((full["triangle"] >= 0).sum()) > 5
    for mask in range(1 << len(names)):
        want = tuple(n for k, n in enumerate(names) if mask >> k & 1)
        alone_or_all_but_one = len(want) in (0, 1, len(names) - 1, len(names))
        got = run_resolve(v, s, zbuf, vertex=src, want=want, plain=not alone_or_all_but_one)
        for n in want:
            assert torch.equal(got[n], full[n]), (want, n)


# ---------------------------------------------------------------------------------------------------------------------
# render_mesh: the shade is the traced surface's
# ---------------------------------------------------------------------------------------------------------------------
def sphere_mesh():
    from oi_amd import mesh
    pos, tris = RR.icosphere(2, RR.SPHERE_RADIUS)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return mesh.IntrinsicMesh(t(pos), t(RR.unit(pos.astype(np.float64))), t(albedo_of(pos)), None, None,
                              triangles=torch.from_numpy(tris).cuda())


BG = (0.1, 0.2, 0.3)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("local", [False, True])
def test_image_is_the_surface_shade_on_the_resolved_arrays(local):
    from oi_amd import ops, raster, trace
    from oi_amd.relight import LocalLight
    gen = G.make_gen("f16x3", 32)
    m = sphere_mesh()
    poses = torch.stack([T.pose("centre"), T.pose("off")])
    lights = [LocalLight(position=(1.5, -1.0, -2.0), radius=0.1), LocalLight(position=(-1.0, 2.0, -1.5))] if local else G.lights()
    outs = raster.render_mesh(gen, m, poses, lights=lights, bg=BG)
    chunks, _, R = raster.rasterise(gen, m, poses)
    (_, w2b, setup, zbuf, g), = chunks
    lt = trace._stack_lights(gen, lights, "cuda", "test")
    shade = ops.surface_shade_local if local else ops.surface_shade
    bg = torch.tensor(BG, device="cuda")
    for e, out in enumerate(outs):
        assert out["stats"]["covered"] > 50 and out["stats"]["triangles"] == 320
        args = [g[k][e] for k in ("rays_o", "rays_d", "t", "status", "hit_slot", "hit_points", "grad", "rgb")]
        mine = shade(*args, R * R, w2b[e], lt, bg, None)
        assert _same(out["image"], mine["image"].view(-1, 3, R, R))
        assert _same(out["depth"], mine["depth"].view(1, 1, R, R)) and _same(out["mask"], mine["mask"].view(1, 1, R, R))
        assert out["image"].shape == (len(lights), 3, R, R) and set(out) == {
            "depth", "position", "normal_map", "normal_object", "albedo", "mask", "image", "triangle", "barycentric", "stats"}
        assert int(out["mask"].sum()) == out["stats"]["covered"] == int((out["triangle"] >= 0).sum())
        assert bool(torch.isnan(out["depth"][out["mask"] == 0]).all())
        # result l of L lights is the 1-light call; a view of E is the single-view call
        for l in (0, len(lights) - 1):
            one = raster.render_mesh(gen, m, poses[e], lights=[lights[l]], bg=BG)
            assert _same(one["image"][0], out["image"][l])
            for k in ("depth", "position", "normal_map", "normal_object", "albedo", "mask", "triangle", "barycentric"):
                assert _same(one[k], out[k]), k
            assert one["stats"] == out["stats"]


def test_mesh_frames_and_resolution():
    from oi_amd import inference, raster
    gen = G.make_gen("f16x3", 32)
    m = sphere_mesh()
    poses = inference.rotation_walk(T.pose("centre"), 5)
    keys = ("image", "mask", "depth", "triangle")
    fr = inference.mesh_frames(gen, m, poses, keys=keys, batch=2)        # groups of 2, 2 and 1
    assert fr["image"].shape == (5, 3, 32, 32) and fr["triangle"].dtype == torch.int32
    for i, b2w in enumerate(poses):
        one = raster.render_mesh(gen, m, b2w)
        for k in keys:
            assert _same(fr[k][i], one[k][0]), k
    # another image side keeps the frustum: the mask's share of the image stays, the depth at the centre too
    big = raster.render_mesh(gen, m, poses[0], resolution=96)
    small = raster.render_mesh(gen, m, poses[0])
    assert big["image"].shape == (1, 3, 96, 96)
    assert abs(float(big["mask"].mean()) - float(small["mask"].mean())) < 0.02
    assert abs(float(big["depth"][0, 0, 48, 48]) - float(small["depth"][0, 0, 16, 16])) < 0.02


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the exported asset, read back from its files, against the traced surface
# ---------------------------------------------------------------------------------------------------------------------
# Measured on one MI355X (f16x3, golden weights, latent 0, lattice 32, crop 32, poses "centre" and "off"; the worst of the two
# poses; 205 and 223 pixels on the common mask).  The quantity is deterministic: the bars stand at 2 x the measured worst
# case -- twice the depth error and the angle, twice the distance of the IoU from 1, twice the RMS error of a PSNR (- 6.02 dB).
# DESIGN section 4.33 has the table.  What the wrong conventions gave in the same run: v not flipped and rows reversed
# 48.8 dB / 48.7 dB of albedo and 100 - 104 degrees of normal; the normal map without its offset 79.5 - 92.7 degrees.
MEASURED = {4: {"mask_iou": 0.990338, "depth_rms": 4.3186e-3, "normal_angle": 0.86094, "albedo_psnr": 60.933, "image_psnr": 44.780},
            8: {"mask_iou": 0.990338, "depth_rms": 4.3186e-3, "normal_angle": 0.48773, "albedo_psnr": 60.031, "image_psnr": 50.960}}
TWICE_DB = 20.0 * np.log10(2.0)


def bars_of(m):
    return {"mask_iou": 1.0 - 2.0 * (1.0 - m["mask_iou"]), "depth_rms": 2.0 * m["depth_rms"], "normal_angle": 2.0 * m["normal_angle"],
            "albedo_psnr": m["albedo_psnr"] - TWICE_DB, "image_psnr": m["image_psnr"] - TWICE_DB}


def _asset(tmp_path, texel):
    from oi_amd import mesh
    gen = G.make_gen("f16x3", 32)
    z = A.latent(0)[0]
    tm = mesh.extract_textured_mesh(gen, z=z.reshape(1, -1).cuda(), resolution=32, texel=texel)
    path = tmp_path / f"asset{texel}.obj"
    mesh.save_obj(str(path), tm)
    return gen, z, tm, mesh.load_obj(str(path))


@pytest.mark.parametrize("texel", [4, 8])
def test_end_to_end_against_the_traced_surface(tmp_path, texel):
    import dataclasses
    from oi_amd import inference
    gen, z, tm, back = _asset(tmp_path, texel)
    assert _same(back.uv, tm.uv) and _same(back.albedo_map, tm.albedo_map) and _same(back.normal_map, tm.normal_map)
    assert _same(back.mesh.triangles, tm.mesh.triangles) and _same(back.mesh.positions, tm.mesh.positions)
    poses = torch.stack([T.pose("centre"), T.pose("off")])
    lights = G.lights()[:1]
    fid = inference.mesh_fidelity(gen, z, back, poses, lights=lights)
    worst = {"mask_iou": min(f["mask_iou"] for f in fid), "depth_rms": max(f["depth_rms"] for f in fid),
             "normal_angle": max(f["normal_angle"] for f in fid), "albedo_psnr": min(f["albedo_psnr"] for f in fid),
             "image_psnr": min(f["image_psnr"] for f in fid)}
    # the negative controls: the same asset read with one convention wrong
    flip_v = back.uv.clone()
    flip_v[..., 1] = 1.0 - flip_v[..., 1]
    controls = {"v_not_flipped": dataclasses.replace(back, uv=flip_v),
                "rows_reversed": dataclasses.replace(back, albedo_map=back.albedo_map.flip(0).contiguous(),
                                                     normal_map=back.normal_map.flip(0).contiguous()),
                "normal_without_offset": dataclasses.replace(back, normal_map=(back.normal_map.float() / 255.0).contiguous())}
    ctl = {k: inference.mesh_fidelity(gen, z, c, poses, lights=lights) for k, c in controls.items()}
    case = f"raster_end_to_end[texel={texel}]"
    for k, val in worst.items():
        record_margin(case, k, val)
    for k, c in ctl.items():
        record_margin(case, k + ":albedo_psnr", max(f["albedo_psnr"] for f in c))
        record_margin(case, k + ":normal_angle", min(f["normal_angle"] for f in c))
    print(case, "worst", worst)
    print(case, "controls", {k: [(round(f["albedo_psnr"], 2), round(f["normal_angle"], 2)) for f in c] for k, c in ctl.items()})
    print(case, "common", [f["common"] for f in fid])
    bars = bars_of(MEASURED[texel])
    assert worst["mask_iou"] >= bars["mask_iou"] and worst["depth_rms"] <= bars["depth_rms"]
    assert worst["normal_angle"] <= bars["normal_angle"]
    assert worst["albedo_psnr"] >= bars["albedo_psnr"] and worst["image_psnr"] >= bars["image_psnr"]
    # each negative control MISSES its bar, in every pose
    for k in ("v_not_flipped", "rows_reversed"):
        assert max(f["albedo_psnr"] for f in ctl[k]) < bars["albedo_psnr"], k
    assert min(f["normal_angle"] for f in ctl["normal_without_offset"]) > bars["normal_angle"]
    # the normals of the first two controls are as wrong as their colours
    for k in ("v_not_flipped", "rows_reversed"):
        assert min(f["normal_angle"] for f in ctl[k]) > bars["normal_angle"], k


def test_texture_beats_vertex_colours_in_image_space():
    """The image-space counterpart of test_gpu_mesh_tex.py::test_texture_beats_vertex_colours, on its mesh (lattice 16, texel
    8) and with its atlas, the FLOAT albedo: rasterised through the texture the albedo is closer to the traced surface's than
    interpolated from the vertices, in both poses.  (The BYTE atlas of the file format carries a quantisation noise of
    1 / (255 sqrt(12)), 58.9 dB: on the golden field, whose albedo is smooth, that is more than the vertex colours' error
    -- 60.9 dB against 71.9 dB at lattice 32 on one MI355X -- so the byte figures are printed, not compared.)"""
    import dataclasses
    from oi_amd import inference, mesh
    gen = G.make_gen("f16x3", 32)
    z = A.latent(0)[0]
    tm = mesh.extract_textured_mesh(gen, z=z.reshape(1, -1).cuda(), resolution=16, texel=8, want_float=True)
    poses = torch.stack([T.pose("centre"), T.pose("off")])
    lights = G.lights()[:1]
    floats = dataclasses.replace(tm, albedo_map=tm.albedo_f32, normal_map=tm.normal_f32)
    tex = inference.mesh_fidelity(gen, z, floats, poses, lights=lights)
    byte = inference.mesh_fidelity(gen, z, tm, poses, lights=lights)
    vertex = inference.mesh_fidelity(gen, z, tm, poses, lights=lights, source="vertex")
    for name, fid in (("texture_f32", tex), ("texture_u8", byte), ("vertex", vertex)):
        record_margin("raster_quality[R=16,texel=8]", name + ":albedo_psnr", min(f["albedo_psnr"] for f in fid))
        print(name, [(round(f["albedo_psnr"], 2), round(f["normal_angle"], 3), round(f["image_psnr"], 2)) for f in fid])
    for a, b in zip(tex, vertex):
        assert a["albedo_psnr"] > b["albedo_psnr"]


# ---------------------------------------------------------------------------------------------------------------------
# no side effects
# ---------------------------------------------------------------------------------------------------------------------
def _forbid(monkeypatch, names, why):
    _, L = _lib()

    def forbidden(*a, **k):
        raise AssertionError(why)
    for n in names:
        monkeypatch.setattr(L, n, forbidden)


def test_traced_and_exported_paths_launch_none_of_the_new_entries(tmp_path, monkeypatch):
    from oi_amd import inference, mesh, trace
    gen = G.make_gen("f16x3", 32)
    z = A.latent(0)[0]
    before = trace.render_surface(gen, z, T.pose("centre"), lights=G.lights())
    _forbid(monkeypatch, ENTRIES, "an entry of include/oi_raster.h ran")
    after = trace.render_surface(gen, z, T.pose("centre"), lights=G.lights())
    assert _same(before["image"], after["image"]) and _same(before["depth"], after["depth"])
    tm = mesh.extract_textured_mesh(gen, z=z.reshape(1, -1).cuda(), resolution=16, texel=4)
    assert len(tm.mesh.triangles) > 100
    out = inference.export_mesh(gen, z, str(tmp_path / "a.obj"), resolution=16, texture=True, texel=4)
    assert _same(out.albedo_map, tm.albedo_map)
    assert isinstance(inference.export_mesh(gen, z, str(tmp_path / "a.ply"), resolution=16), mesh.IntrinsicMesh)


def test_render_mesh_launches_no_mlp_entry(monkeypatch):
    from oi_amd import lib, raster
    gen = G.make_gen("f16x3", 32)
    m = sphere_mesh()
    plain = raster.render_mesh(gen, m, T.pose("centre"))
    names = [n for entries in lib.SIGS.values() for n in entries if n.startswith("oi_sdf_mlp_") or n.startswith("oi_color_head")]
    assert "oi_sdf_mlp_fwd" in names and "oi_sdf_mlp_fwd_segments" in names
    _forbid(monkeypatch, names, "render_mesh launched an MLP entry")
    again = raster.render_mesh(gen, m, T.pose("centre"))
    assert _same(plain["image"], again["image"]) and plain["stats"] == again["stats"]


def test_refusals_on_the_device():
    from oi_amd import mesh, raster
    gen = G.make_gen("f16x3", 32)
    m = sphere_mesh()
    bad = mesh.IntrinsicMesh(m.positions, m.normals, m.albedo, None, None, triangles=m.triangles.clone())
    bad.triangles[7, 1] = len(m.positions)
    with pytest.raises(ValueError, match="triangle indices 0 .. 162 outside the mesh's 162 vertices"):
        raster.render_mesh(gen, bad, T.pose("centre"))
    empty = mesh.IntrinsicMesh(m.positions, m.normals, m.albedo, None, None, triangles=m.triangles[:0].contiguous())
    out = raster.render_mesh(gen, empty, T.pose("centre"), bg=BG)        # no triangle: the background, nothing fails
    assert out["stats"] == {"triangles": 0, "dropped": 0, "empty": 0, "small": 0, "large": 0, "covered": 0}
    assert float(out["mask"].sum()) == 0 and bool((out["triangle"] == -1).all())
    lib, L = _lib()
    v = Views([RR.camera(7, 0)])
    s = run_setup(v, *RR.quad())
    for args, text in (((7, 0), "E=0 views"), ((0, 1), "resolution R=0"), ((16385, 1), "resolution R=16385")):
        rc = L.oi_raster_fill(_p(v.c2b), _p(v.kinv), _p(v.offs), args[0], args[1], _p(s["pos"]), _p(s["tris"]), 4, 2,
                              _p(s["corners"]), _p(s["bbox"]), _p(s["small_list"]), _p(s["large_list"]), _p(s["counts"]),
                              _p(s["corners"]), None)
        assert rc < 0 and text in L.oi_last_error().decode()
    rc = L.oi_raster_setup(_p(v.b2c), _p(v.K), _p(v.offs), 7, 1, _p(s["pos"]), _p(s["tris"]), 4, 2, 0.0, 16,
                           *(_p(s[k]) for k in ("corners", "bbox", "cls", "small_list", "large_list", "counts")), None)
    assert rc < 0 and "near=0" in L.oi_last_error().decode()
