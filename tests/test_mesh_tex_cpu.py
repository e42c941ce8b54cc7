"""CPU checks of the textured mesh export (include/oi_mesh_tex.h; oi_amd.mesh.bake_textures / save_png / save_obj;
oi_amd.inference.export_mesh(texture=True)): header <=> library <=> binding, oi_tex_layout against the
restatement of tests/helpers/mesh_tex_ref.py, the ownership of the atlas' pixels, the safety of bilinear lookups, the file
writers, the host's argument checks, and the REHEARSAL on the fp64 oracle alone of what tests/test_gpu_mesh_tex.py asserts.

Rehearsal results (oracle alone, float64, golden weights, bounds [-1, 1]^3, refine = 2, texel 8, 2000 seeded surface samples;
error = largest channel difference of the albedo to the oracle albedo at the sample's Newton projection, median):

    R    seed   F      texture (a)   vertex colours (b)   (b) / (a)
    16   0      620    3.97e-5       6.29e-4              15.9
    16   1      620    4.01e-5       6.25e-4              15.6
    24   0      1360   1.81e-5       3.37e-4              18.6
    24   1      1380   1.84e-5       3.59e-4              19.6
    32   0      2484   9.56e-6       2.04e-4              21.3
    32   1      2492   1.00e-5       2.08e-4              20.7

so the smallest of {16, 24, 32} at which (b) is at least 4 x (a) is 16: the resolution of
test_gpu_mesh_tex.py::test_texture_beats_vertex_colours.  The limit band (texels whose Newton candidate comes within 1e-4
relative of the half-cell limit, R = 32, seeded subsample of 20000 texels): no texel at texel 4 or 8, seeds 0 and 1, and no
texel flagged -- under the 1 % the flag comparison of the GPU test needs."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from helpers import cabi
from helpers import mesh_tex_ref as X

FS = (0, 1, 2, 3, 7, 8, 9, 10001)
TS = (3, 4, 5, 8, 64)
KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
_lib = cabi.built_lib


def _layout(L, F, T):
    W, H, cols = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = L.oi_tex_layout(F, T, ctypes.byref(W), ctypes.byref(H), ctypes.byref(cols))
    return rc, W.value, H.value, cols.value


def test_header_contract_and_layout():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_mesh_tex.h", lib)
    assert names == ["oi_tex_layout", "oi_tex_uv", "oi_tex_points", "oi_tex_store"] and mirrors == []
    text = cabi.read("oi_mesh_tex.h")
    assert "struct" not in text.split("#ifndef OI_MESH_TEX_H_")[1]
    for macro, val in (("OI_TEX_MIN_TEXEL", lib.TEX_MIN_TEXEL), ("OI_TEX_MAX_TEXEL", lib.TEX_MAX_TEXEL),
                       ("OI_TEX_MAX_SIZE", lib.TEX_MAX_SIZE)):
        assert f"#define {macro} {val}\n" in text
    assert (lib.TEX_MIN_TEXEL, lib.TEX_MAX_TEXEL, lib.TEX_MAX_SIZE) == (X.MIN_TEXEL, X.MAX_TEXEL, X.MAX_SIZE) == (3, 64, 16384)
    from conftest import ROOT
    assert '"mesh_tex.hip"' in open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    from oi_amd import ops
    for F in FS:
        for T in TS:
            W, H, cols, rows = X.layout(F, T)
            assert _layout(L, F, T) == (0, W, H, cols), (F, T)
            assert ops.tex_layout(F, T) == (W, H, cols)
            assert cols * cols >= (F + 1) // 2 and (cols - 1) ** 2 < max((F + 1) // 2, 1) and cols * rows >= (F + 1) // 2
    assert X.layout(0, 8)[:2] == (9, 8) and X.layout(10001, 8) == (71 * 9, 71 * 8, 71, 71)
    # refusals: the texel size, the triangle count, an atlas over the limit (its size is still reported)
    for T in (2, 65, 0, -1):
        assert _layout(L, 10, T)[0] == -1 and "texel size" in L.oi_last_error().decode()
        with pytest.raises(ValueError, match="texel"):
            ops.tex_layout(10, T)
    assert _layout(L, -1, 8)[0] == -1 and _layout(L, 1 << 31, 8)[0] == -1
    F = 2 * 253 * 253                                # 253 columns of 65 texels = 16445 > 16384
    assert X.layout(F, 64)[0] == 253 * 65
    rc, W, H, cols = _layout(L, F, 64)
    assert rc == -1 and (W, H, cols) == (253 * 65, 253 * 64, 253) and "smaller texel" in L.oi_last_error().decode()
    with pytest.raises(ValueError, match="smaller texel"):
        ops.tex_layout(F, 64)
    assert _layout(L, 2 * 252 * 252, 64)[0] == 0     # 16380 x 16128
    assert L.oi_tex_layout(7, 8, None, None, None) == 0


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    cases = [(lambda: L.oi_tex_uv(5, 2, f, None), "oi_tex_layout", "texel size"),
             (lambda: L.oi_tex_uv(-1, 8, f, None), "oi_tex_layout", "F=-1"),
             (lambda: L.oi_tex_uv(5, 8, None, None), "oi_tex_uv", "null"),
             (lambda: L.oi_tex_points(f, f, 0, 5, 65, f, f, None), "oi_tex_points", "texel size"),
             (lambda: L.oi_tex_points(f, f, -1, 5, 8, f, f, None), "oi_tex_points", "chunk"),
             (lambda: L.oi_tex_points(f, f, 0, (1 << 31) // 36 + 1, 8, f, f, None), "oi_tex_points", "2^31"),
             (lambda: L.oi_tex_points(None, f, 0, 5, 8, f, f, None), "oi_tex_points", "null"),
             (lambda: L.oi_tex_points(f, None, 0, 5, 8, f, f, None), "oi_tex_points", "null"),
             (lambda: L.oi_tex_points(f, f, 0, 5, 8, None, f, None), "oi_tex_points", "null"),
             (lambda: L.oi_tex_store(f, f, 0, 5, 2, 9, f, f, f, f, None), "oi_tex_store", "texel size"),
             (lambda: L.oi_tex_store(f, f, 5, 5, 8, 9, f, f, f, f, None), "oi_tex_store", "past the mesh"),
             (lambda: L.oi_tex_store(None, f, 0, 5, 8, 9, f, f, f, f, None), "oi_tex_store", "null"),
             (lambda: L.oi_tex_store(f, None, 0, 5, 8, 9, None, None, f, None, None), "oi_tex_store", "null")]
    for call, entry, text in cases:
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)
    # nothing to do: success, nothing launched (null buffers are fine)
    assert L.oi_tex_uv(0, 8, None, None) == 0
    assert L.oi_tex_points(None, None, 0, 0, 8, None, None, None) == 0
    assert L.oi_tex_store(None, None, 0, 0, 8, 0, None, None, None, None, None) == 0
    assert L.oi_tex_store(None, None, 0, 5, 8, 9, None, None, None, None, None) == 0     # every atlas optional


@pytest.mark.parametrize("T", TS)
def test_ownership(T):
    """The pixels of all (f, k) are distinct and inside W x H; with the unowned half-cell (odd F) and the tail cells they
    cover the image exactly once."""
    i, j = X.texel_ij(T)
    assert len(i) == X.n_texels(T) and (i + j <= T - 1).all() and (i >= 0).all() and (j >= 0).all()
    for F in FS:
        W, H, cols, rows = X.layout(F, T)
        px = X.pixels(F, T).reshape(-1, 2)
        assert len(px) == F * X.n_texels(T)
        count = np.zeros((H, W), dtype=np.int64)
        if F:
            assert px.min() >= 0 and px[:, 0].max() < W and px[:, 1].max() < H
            np.add.at(count, (px[:, 1], px[:, 0]), 1)
        assert count.max(initial=0) <= 1                              # distinct
        if F & 1:                                                     # the upper half of the last cell: no owner
            ghost = X.pixels(F + 1, T, [F])[0] if X.layout(F + 1, T)[:3] == (W, H, cols) else None
            assert ghost is not None
            assert (count[ghost[:, 1], ghost[:, 0]] == 0).all()
            count[ghost[:, 1], ghost[:, 0]] += 1
        ncells = (F + 1) >> 1
        for c in range(ncells, cols * rows):                          # the tail cells
            x0, y0 = (c % cols) * (T + 1), (c // cols) * T
            assert (count[y0:y0 + T, x0:x0 + T + 1] == 0).all()
            count[y0:y0 + T, x0:x0 + T + 1] += 1
        assert (count == 1).all()


@pytest.mark.parametrize("T", [3, 4, 5, 8])
def test_bilinear_lookups_stay_inside_the_triangle(T):
    """Every tap with non-zero weight of a bilinear lookup anywhere in the closed UV triangle is a texel of that triangle: a
    barycentric grid of 24 steps per edge, edges and corners included, every triangle of an F = 9 atlas."""
    F, n = 9, 24
    W, H, _, _ = X.layout(F, T)
    owner = np.full((H, W), -1, dtype=np.int64)
    px = X.pixels(F, T)
    for f in range(F):
        owner[px[f, :, 1], px[f, :, 0]] = f
    grid = np.array([(a, b, n - a - b) for a in range(n + 1) for b in range(n + 1 - a)], dtype=np.float64) / n
    assert len(grid) == (n + 1) * (n + 2) // 2
    cuv = X.corner_uv(F, T)
    for f in range(F):
        uv = grid @ cuv[f]
        taps, wts = X.bilinear_taps(uv, W, H)
        # weights that are zero but for the rounding of u * W (a lookup exactly on a texel centre) carry nothing
        live = wts > 1e-9
        assert live.any(1).all()
        tx, ty = taps[..., 0][live], taps[..., 1][live]
        assert tx.min() >= 0 and tx.max() < W and ty.min() >= 0 and ty.max() < H
        assert (owner[ty, tx] == f).all(), (T, f)
        # and the lookup reproduces a function that is linear over the triangle's own texels
        lin = np.zeros((H, W, 1))
        b = X.barycentrics(T)
        lin[px[f, :, 1], px[f, :, 0], 0] = b @ np.array([1.0, 2.0, 4.0])
        assert np.abs(X.sample_bilinear(lin, uv)[:, 0] - grid @ np.array([1.0, 2.0, 4.0])).max() < 1e-9


def _decode_png(data):
    """A PNG reader for 8-bit RGB, filter type 0, from zlib and struct alone."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 3)


def test_save_png(tmp_path):
    from oi_amd import mesh
    rs = np.random.RandomState(0)
    for shape in ((8, 9, 3), (1, 1, 3), (37, 5, 3)):
        img = rs.randint(0, 256, shape).astype(np.uint8)
        p, q = str(tmp_path / "a.png"), str(tmp_path / "b.png")
        mesh.save_png(p, img)
        mesh.save_png(q, torch.from_numpy(img))
        data = open(p, "rb").read()
        assert data == open(q, "rb").read()                            # the same input, the same bytes
        assert np.array_equal(_decode_png(data), img)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="save_png"):
            mesh.save_png(str(tmp_path / "bad.png"), bad)


def test_save_png_reads_back_with_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from oi_amd import mesh
    img = np.random.RandomState(1).randint(0, 256, (16, 27, 3)).astype(np.uint8)
    p = str(tmp_path / "a.png")
    mesh.save_png(p, img)
    with Image.open(p) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


def _textured(F=5, T=4, seed=0):
    from oi_amd import mesh
    rs = np.random.RandomState(seed)
    V = F + 2
    pos = (rs.rand(V, 3) * 2.4 - 1.2).astype(np.float32)
    nrm = rs.randn(V, 3).astype(np.float32)
    tris = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], -1).astype(np.int32)
    W, H, _, _ = X.layout(F, T)
    m = mesh.IntrinsicMesh(torch.from_numpy(pos), torch.from_numpy(nrm), torch.zeros(V, 3), torch.zeros(3, V),
                           torch.zeros(V, dtype=torch.uint8), triangles=torch.from_numpy(tris))
    uv = X.corner_uv(F, T).astype(np.float32)
    maps = [torch.from_numpy(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)) for _ in range(2)]
    nT = X.n_texels(T)
    return mesh.TexturedMesh(m, torch.from_numpy(uv), maps[0], maps[1], T, (W, H), torch.zeros(F, nT, dtype=torch.uint8),
                             torch.zeros(F, nT)), pos, nrm, tris, uv


def test_save_obj(tmp_path):
    from oi_amd import mesh
    tm, pos, nrm, tris, uv = _textured()
    path = tmp_path / "rose.obj"
    mesh.save_obj(str(path), tm)
    assert sorted(os.listdir(tmp_path)) == ["rose.mtl", "rose.obj", "rose_albedo.png", "rose_normal.png"]
    rows = {"v": [], "vn": [], "vt": [], "f": []}
    head = []
    for ln in path.read_text().splitlines():
        tok = ln.split()
        (rows[tok[0]] if tok[0] in rows else head).append(tok[1:])
    assert head == [["rose.mtl"], ["intrinsic"]]
    F = len(tris)
    assert np.array_equal(np.array(rows["v"], dtype=np.float64).astype(np.float32), pos)          # bit-equal as float32
    assert np.array_equal(np.array(rows["vn"], dtype=np.float64).astype(np.float32), nrm)
    assert len(rows["vt"]) == 3 * F
    assert np.array_equal(np.array(rows["vt"], dtype=np.float64).astype(np.float32), uv.reshape(-1, 2))
    faces = np.array([[[int(x) for x in c.split("/")] for c in r] for r in rows["f"]])            # (F, 3, 3), 1-based
    assert faces.shape == (F, 3, 3) and faces.min() == 1
    assert np.array_equal(faces[..., 0] - 1, tris) and np.array_equal(faces[..., 2], faces[..., 0])
    assert np.array_equal(faces[..., 1] - 1, np.arange(3 * F).reshape(F, 3))
    assert (tmp_path / "rose.mtl").read_text().split("\n") == ["newmtl intrinsic", "Kd 1 1 1", "map_Kd rose_albedo.png",
                                                               "norm rose_normal.png", ""]
    assert np.array_equal(_decode_png((tmp_path / "rose_albedo.png").read_bytes()), tm.albedo_map.numpy())
    assert np.array_equal(_decode_png((tmp_path / "rose_normal.png").read_bytes()), tm.normal_map.numpy())
    lit = torch.full_like(tm.albedo_map, 7)
    mesh.save_obj(str(path), tm, light_map=lit)
    assert np.array_equal(_decode_png((tmp_path / "rose_albedo.png").read_bytes()), lit.numpy())
    with pytest.raises(ValueError, match=r"\.obj"):
        mesh.save_obj(str(tmp_path / "rose.ply"), tm)


def test_host_validation_launches_nothing(tmp_path, monkeypatch):
    """A bad texel, texture=True with a .ply path and a triangle index >= V each raise ValueError before any launch: the
    launching entries are replaced by ones that fail the test, and every tensor is on the CPU."""
    from oi_amd import inference, lib, mesh
    from oi_amd.fields import ColorNetwork, FieldPack, ShapeNetwork
    L = lib.load()

    def forbidden(*a, **k):
        raise AssertionError("an entry of include/oi_mesh_tex.h was launched")
    for name in ("oi_tex_uv", "oi_tex_points", "oi_tex_store"):
        monkeypatch.setattr(L, name, forbidden)
    monkeypatch.setattr(mesh, "extract_intrinsic_mesh", forbidden)
    pack = FieldPack(ShapeNetwork(None, **KW), ColorNetwork(**KW))
    tm, _, _, tris, _ = _textured()
    z = torch.zeros(1, 64)
    box = ((-1.0,) * 3, (1.0,) * 3, 16)
    for bad in (2, 65, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="texel"):
            mesh.bake_textures(pack, tm.mesh, *box, z=z, texel=bad)
        with pytest.raises(ValueError, match="texel"):
            mesh.extract_textured_mesh(pack, z=z, resolution=16, texel=bad)
    for bad in (0, -1, 1.5, 1 << 31):
        with pytest.raises(ValueError, match="max_texels"):
            mesh.bake_textures(pack, tm.mesh, *box, z=z, max_texels=bad)
    with pytest.raises(ValueError, match="refine"):
        mesh.bake_textures(pack, tm.mesh, *box, z=z, refine=9)
    with pytest.raises(ValueError, match="latent"):
        mesh.bake_textures(pack, tm.mesh, *box)
    V = len(tm.mesh.positions)
    for bad in (V, V + 5, -1):
        t = tris.copy()
        t[3, 1] = bad
        tm.mesh.triangles = torch.from_numpy(t)
        with pytest.raises(ValueError, match=f"the mesh has {V} vertices"):
            mesh.bake_textures(pack, tm.mesh, *box, z=z)
    tm.mesh.triangles = None
    with pytest.raises(ValueError, match="triangles"):
        mesh.bake_textures(pack, tm.mesh, *box, z=z)
    tm.mesh.triangles = torch.from_numpy(tris)
    with pytest.raises(lib.OiHipError):                                   # no CPU path
        mesh.bake_textures(pack, tm.mesh, *box, z=z)
    # export_mesh(texture=True): the path and the texel size are looked at before the generator is
    for path in ("rose.ply", "rose", "rose.obj.ply"):
        with pytest.raises(ValueError, match=r"\.obj"):
            inference.export_mesh(None, z, str(tmp_path / path), texture=True)
    with pytest.raises(ValueError, match="texel"):
        inference.export_mesh(None, z, str(tmp_path / "rose.obj"), texture=True, texel=2)
    assert os.listdir(tmp_path) == []


def test_quantisation_restatement():
    c = np.array([0.0, 1.0, 0.5, 1.5, -0.2, np.nan, 0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255, np.inf, -np.inf],
                 dtype=np.float32)
    assert X.quant8(c).tolist() == [0, 255, 128, 255, 0, 0, 0, 2, 2, 254, 255, 0]


def test_rehearsal_of_the_quality_condition():
    """On the oracle alone (an atlas built by the fp64 restatement): at texel 8 the barycentric interpolation of the vertex
    albedo is at least 4 x as far from the field as the bilinear lookup of the texture already at R = 16, the smallest of the
    resolutions {16, 24, 32} -- the resolution test_gpu_mesh_tex.py::test_texture_beats_vertex_colours uses."""
    ea, eb, F = X.rehearse_quality(0, 16, 8)
    print("rehearsal R=16 texel=8: texture", ea, "vertex colours", eb, "F", F)
    assert F > 200 and eb >= 4 * ea


def test_rehearsal_of_the_limit_band():
    """The texels of an R = 32 mesh whose Newton candidate comes within 1e-4 (relative) of the half-cell limit: under 1 % on
    the oracle alone, so the flag comparison of the GPU test leaves out almost nothing."""
    for T in (4, 8):
        near, flagged = X.rehearse_band(0, 32, T, n=4000)
        print("rehearsal R=32 texel", T, "near the limit", near, "flagged", flagged)
        assert near < 0.01
