"""The mesh rasteriser without a GPU (include/oi_raster.h; oi_amd.raster): the integer reference of
tests/helpers/raster_ref.py against a brute-force caster, the coverage rule on shared edges and a closed fan, what the
float64 reference alone gives for the conditions tests/test_gpu_raster.py sets, the Python refusals, and the file-level
round trip save_obj -> load_obj."""
import struct
import types
import zlib

import numpy as np
import pytest
import torch

from helpers import raster_ref as RR

NEAR, SMALL_MAX = 1e-3, 16


def _reference(cam, pos, tris):
    corners, fixed, cls, bbox = RR.setup(cam, pos, tris, NEAR, SMALL_MAX)
    return corners, fixed, cls, bbox, RR.raster(cam, pos, tris, corners, cls, bbox)


# The condition: at most 2 % of the covered centres lie within one fixed-point unit of an edge.  64 triangles have 192 edges of
# a few pixels each, so about 8 of some 300 covered centres do on average: of the seeds 0 .. 11 (camera s on soup s) the seeds
# 1, 5, 9 and 11 stay under the 2 % on the reference pair itself (2, 5, 5 and 5 centres; printed below) and are the ones used.
@pytest.mark.parametrize("case", ["soup1", "soup5", "soup9", "soup11"])
def test_integer_reference_is_the_caster_away_from_edges(case):
    s = int(case[4:])
    cam, (pos, tris) = RR.camera(33, s), RR.soup(64, s)
    corners, fixed, cls, bbox, (ids, t, _, _, _) = _reference(cam, pos, tris)
    cids, ct = RR.cast(cam, pos, tris)
    edge = RR.near_edge(cam, fixed, cls, bbox, 1.0)
    covered = (ids >= 0) | (cids >= 0)
    share = float((edge & covered).sum()) / float(covered.sum())
    print(case, "covered", int(covered.sum()), "near an edge", int((edge & covered).sum()), f"{share:.4f}")
    assert covered.sum() > 100 and share <= 0.02
    assert np.array_equal(ids[~edge], cids[~edge])
    both = ~edge & (ids >= 0)
    assert np.abs(t[both] - ct[both]).max() < 1e-12


def _count(corner_sets, X, Y):
    return sum(RR.covers_int(c, X, Y) for c in corner_sets)


@pytest.mark.parametrize("flip", [False, True])
def test_shared_edge_covers_each_centre_once(flip):
    """A square of 8 x 8 pixels whose diagonal runs THROUGH the centres (k, k), and whose outline runs through centres too:
    every centre inside, and every one on the diagonal, is covered exactly once in either orientation; the outline's centres
    at most once."""
    a, b = RR.tie_square(flip)
    for Y in range(-1, 10):
        for X in range(-1, 10):
            n = _count([a, b], X, Y)
            if 0 < X < 8 and 0 < Y < 8:
                assert n == 1, (X, Y, n)
            else:
                assert n <= 1 and (n == 0 or (0 <= X <= 8 and 0 <= Y <= 8)), (X, Y, n)
    # the top-left rule itself: the top and the left outline are owned, the bottom and the right are not
    assert _count([a, b], 3, 0) == 1 and _count([a, b], 0, 3) == 1 and _count([a, b], 3, 8) == 0 and _count([a, b], 8, 3) == 0


def test_closed_fan_covers_each_centre_once():
    """A fan about an apex that IS a pixel centre, rim corners on centres and between them, mixed orientations."""
    tris, rim = RR.tie_fan()
    outline = np.array(rim, dtype=np.float64)
    total = 0
    for Y in range(0, 13):
        for X in range(0, 13):
            n = _count(tris, X, Y)
            assert n <= 1
            # strictly inside the rim polygon (orientation test against every rim edge)
            p = np.array([X * RR.FIX, Y * RR.FIX], dtype=np.float64)
            e, w = np.roll(outline, -1, 0) - outline, p - outline
            if (e[:, 0] * w[:, 1] - e[:, 1] * w[:, 0] > 0).all():
                assert n == 1, (X, Y)
                total += 1
    assert total > 60 and _count(tris, 6, 6) == 1


def test_the_conditions_of_the_gpu_tests_hold_on_the_reference_alone():
    """What tests/test_gpu_raster.py may assume, shown on the float64 reference: on the soup at most 2 % of the covered pixels
    have their two nearest candidates within the depth bar (they are left unexamined); on the sphere no pixel has, at most
    5 % of the covered pixels are grazing (|n . d| < 0.05), and the faceted sphere lies within the sag of its faces under
    the analytic one (raster_ref.face_sag has the derivation)."""
    cam, pos, tris = RR.soup_case()
    *_, (ids, t, second, cosine, count) = _reference(cam, pos, tris)
    left = RR.unexamined(t, second, cosine)
    covered = int((ids >= 0).sum())
    print("soup: covered", covered, "unexamined", int(left.sum()), "overlapped", int((count > 1).sum()))
    assert covered > 250 and (count > 1).sum() > 100 and left.sum() <= 0.02 * covered

    cam, pos, tris = RR.sphere_case()
    *_, (ids, t, second, cosine, count) = _reference(cam, pos, tris)
    covered = int((ids >= 0).sum())
    grazing = (ids >= 0) & (cosine < RR.GRAZING)
    print("sphere: covered", covered, "grazing", int(grazing.sum()), "unexamined", int(RR.unexamined(t, second, cosine).sum()))
    assert covered > 300 and grazing.sum() <= 0.05 * covered and not RR.unexamined(t, second, cosine).any()
    radial, along, ok = RR.sphere_gaps(cam, t, RR.SPHERE_RADIUS)
    on = (ids >= 0) & ~grazing
    sag = RR.face_sag(RR.SPHERE_RADIUS, RR.longest_edge(pos, tris))
    assert (radial[on] >= -1e-12).all() and (radial[on] <= sag + 1e-12).all()
    bound = RR.along_ray_bound(cam, RR.SPHERE_RADIUS, sag)
    assert (along[on & ok] >= -1e-12).all() and (along[on & ok] <= bound[on & ok] + 1e-12).all()
    # the sag under an EDGE's midpoint, r - sqrt(r^2 - (h / 2)^2), is NOT a bound of a face: the exact
    # float64 mesh already lies deeper than it under the faces' centroids
    edge_sag = RR.SPHERE_RADIUS - np.sqrt(RR.SPHERE_RADIUS ** 2 - (RR.longest_edge(pos, tris) / 2) ** 2)
    print("sphere: radial depth", float(radial[on].max()), "face sag", sag, "edge sag", edge_sag)
    assert radial[on].max() > edge_sag


def test_setup_classes_on_the_reference():
    """The class rules on hand-made corners: zero area, off the screen, between the centres, exactly small_max and one more."""
    R = 7
    c = lambda *p: np.array(p, dtype=np.int64) * 1
    F = RR.FIX
    cases = [(c((0, 0), (F, F), (2 * F, 2 * F)), RR.EMPTY),                          # zero area
             (c((-5 * F, 0), (-3 * F, 0), (-4 * F, 2 * F)), RR.EMPTY),               # left of the screen
             (c((F + 10, F + 10), (F + 200, F + 20), (F + 100, F + 220)), RR.EMPTY),  # between the centres
             (c((0, 0), (3 * F, 0), (0, 3 * F)), RR.SMALL),                          # a box of 4 x 4 = 16 centres
             (c((0, 0), (4 * F, 0), (0, 3 * F)), RR.LARGE),                          # 5 x 4 = 20
             (c((-20 * F, -20 * F), (40 * F, -20 * F), (-20 * F, 40 * F)), RR.LARGE)]  # larger than the screen
    corners = np.stack([k for k, _ in cases])
    cls, bbox = RR.classify(corners, np.ones(len(cases), dtype=bool), R, SMALL_MAX)
    assert cls.tolist() == [k for _, k in cases]
    assert bbox[3].tolist() == [0, 0, 3, 3] and bbox[5].tolist() == [0, 0, R - 1, R - 1] and bbox[0].tolist() == [0, 0, -1, -1]


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def _mesh(F=2, triangles=True):
    from oi_amd import mesh
    pos, tris = RR.quad()
    e = torch.zeros(len(pos), 3)
    return mesh.IntrinsicMesh(torch.from_numpy(pos), e + 1, e, None, None, triangles=torch.from_numpy(tris) if triangles else None)


def _gen(R=8):
    return types.SimpleNamespace(it=torch.zeros(1), resolution=R, eval=lambda: None)


def test_python_refusals():
    from oi_amd import raster
    from oi_amd.relight import Light
    pose = torch.eye(4)
    light = Light(direction=(0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="no triangles"):
        raster.render_mesh(_gen(), _mesh(triangles=False), pose, lights=[light])
    with pytest.raises(ValueError, match="source='texture' needs a TexturedMesh"):
        raster.render_mesh(_gen(), _mesh(), pose, lights=[light], source="texture")
    with pytest.raises(ValueError, match="source='mip'"):
        raster.render_mesh(_gen(), _mesh(), pose, lights=[light], source="mip")
    with pytest.raises(TypeError, match="IntrinsicMesh or TexturedMesh"):
        raster.render_mesh(_gen(), object(), pose, lights=[light])
    bad = pose.clone()
    bad[0, 3] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        raster.render_mesh(_gen(), _mesh(), bad, lights=[light])
    with pytest.raises(ValueError, match="expected one \\(4, 4\\) pose"):
        raster.render_mesh(_gen(), _mesh(), torch.eye(3), lights=[light])
    with pytest.raises(ValueError, match="257 lights"):
        raster.render_mesh(_gen(), _mesh(), pose, lights=[light] * 257)
    with pytest.raises(ValueError, match="E \\* R \\* R < 2\\^31"):
        raster.render_mesh(_gen(), _mesh(), torch.eye(4).expand(9, 4, 4), lights=[light], resolution=16384)
    with pytest.raises(ValueError, match="resolution=0"):
        raster.render_mesh(_gen(), _mesh(), pose, lights=[light], resolution=0)
    with pytest.raises(ValueError, match="near=0"):
        raster.render_mesh(_gen(), _mesh(), pose, lights=[light], near=0)
    with pytest.raises(Exception, match="no CPU path"):                   # a mesh that is not on the GPU
        raster.render_mesh(_gen(), _mesh(), pose, lights=[light])
    from oi_amd import inference
    with pytest.raises(ValueError, match="batch=0"):
        inference.mesh_frames(_gen(), _mesh(), [pose], batch=0)
    with pytest.raises(ValueError, match="keys \\['visibility'\\]"):
        inference.mesh_frames(_gen(), _mesh(), [pose], keys=("visibility",))


def test_header_is_bound_without_a_struct():
    from helpers import cabi
    from oi_amd import lib
    assert lib.symbols("oi_raster.h") == ["oi_raster_fill", "oi_raster_resolve", "oi_raster_setup"]
    protos, structs = cabi.parse(cabi.read("oi_raster.h"))
    assert sorted(protos) == lib.symbols("oi_raster.h") and structs == {}
    for name, (res, args) in lib.SIGS["oi_raster.h"].items():
        assert len(args) == len(protos[name][1])
        assert not any(isinstance(a, type) and hasattr(a, "_type_") and hasattr(a._type_, "_fields_") for a in args)
    assert (lib.RASTER_DROPPED, lib.RASTER_EMPTY, lib.RASTER_SMALL, lib.RASTER_LARGE) == (RR.DROPPED, RR.EMPTY, RR.SMALL, RR.LARGE)
    text = cabi.read("oi_raster.h")
    for name, value in (("OI_RASTER_MAX_VIEWS", lib.RASTER_MAX_VIEWS), ("OI_RASTER_MAX_RESOLUTION", lib.RASTER_MAX_RESOLUTION),
                        ("OI_RASTER_MAX_COORD", lib.RASTER_MAX_COORD), ("OI_RASTER_VERTEX", lib.RASTER_VERTEX),
                        ("OI_RASTER_TEXTURE", lib.RASTER_TEXTURE)):
        assert f"#define {name} {value}" in text


# ---------------------------------------------------------------------------------------------------------------------
# the files
# ---------------------------------------------------------------------------------------------------------------------
def _textured(seed=0, F=5, H=9, W=14):
    from oi_amd import mesh
    rs = np.random.RandomState(seed)
    V = F + 2
    pos = torch.from_numpy((rs.rand(V, 3) * 2 - 1).astype(np.float32))
    nrm = torch.from_numpy(rs.randn(V, 3).astype(np.float32))
    tris = torch.from_numpy(np.stack([rs.permutation(V)[:3] for _ in range(F)]).astype(np.int32))
    uv = torch.from_numpy(rs.rand(F, 3, 2).astype(np.float32))
    maps = [torch.from_numpy(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)) for _ in range(2)]
    m = mesh.IntrinsicMesh(pos, nrm, torch.zeros(V, 3), None, None, triangles=tris)
    return mesh.TexturedMesh(m, uv, maps[0], maps[1], 4, (W, H), None, None)


def test_load_obj_round_trips_save_obj(tmp_path):
    from oi_amd import mesh
    tm = _textured()
    path = tmp_path / "asset.obj"
    mesh.save_obj(str(path), tm)
    back = mesh.load_obj(str(path), device="cpu")
    for got, exp in ((back.uv, tm.uv), (back.mesh.triangles, tm.mesh.triangles), (back.albedo_map, tm.albedo_map),
                     (back.normal_map, tm.normal_map), (back.mesh.positions, tm.mesh.positions), (back.mesh.normals, tm.mesh.normals)):
        assert got.dtype == exp.dtype and got.shape == exp.shape and got.numpy().tobytes() == exp.numpy().tobytes()
    assert back.size == tm.size and back.mesh.albedo is None and back.texel is None
    # a second save of what was read gives the same four files
    again = tmp_path / "again.obj"
    mesh.save_obj(str(again), back)
    assert (tmp_path / "again_albedo.png").read_bytes() == (tmp_path / "asset_albedo.png").read_bytes()
    assert again.read_text() == path.read_text().replace("asset", "again")


def _png(W, H, depth, colour, interlace, rows):
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace)) +
            chunk(b"IDAT", zlib.compress(rows)) + chunk(b"IEND", b""))


def test_load_obj_refuses_what_save_obj_does_not_write(tmp_path):
    from oi_amd import mesh
    tm = _textured(F=1, H=2, W=2)
    path = tmp_path / "a.obj"

    def saved():
        mesh.save_obj(str(path), tm)
        return tmp_path / "a_albedo.png"
    row8 = b"\0" + bytes(6)
    saved().write_bytes(_png(2, 2, 8, 2, 1, row8 * 2))
    with pytest.raises(ValueError, match="interlaced"):
        mesh.load_obj(str(path), device="cpu")
    saved().write_bytes(_png(2, 2, 16, 2, 0, (b"\0" + bytes(12)) * 2))
    with pytest.raises(ValueError, match="bit depth 16"):
        mesh.load_obj(str(path), device="cpu")
    saved().write_bytes(_png(2, 2, 8, 6, 0, (b"\0" + bytes(8)) * 2))
    with pytest.raises(ValueError, match="colour type 6"):
        mesh.load_obj(str(path), device="cpu")
    saved().write_bytes(_png(2, 2, 8, 2, 0, (b"\1" + bytes(6)) * 2))
    with pytest.raises(ValueError, match="row filter type 1"):
        mesh.load_obj(str(path), device="cpu")
    saved()
    path.write_text(path.read_text() + "l 1 2\n")
    with pytest.raises(ValueError, match="unsupported statement 'l 1 2'"):
        mesh.load_obj(str(path), device="cpu")
    saved()
    path.write_text(path.read_text().replace("f 1/1/1", "f 1/1/2", 1) if "f 1/1/1" in path.read_text() else
                    path.read_text().replace("/1/", "//", 1))
    with pytest.raises(ValueError, match="only v/vt/vn corners"):
        mesh.load_obj(str(path), device="cpu")
    saved()
    (tmp_path / "a.mtl").write_text((tmp_path / "a.mtl").read_text() + "map_Ks spec.png\n")
    with pytest.raises(ValueError, match="unsupported statement 'map_Ks spec.png'"):
        mesh.load_obj(str(path), device="cpu")
    with pytest.raises(ValueError, match="must end in .obj"):
        mesh.load_obj(str(tmp_path / "a.ply"))
