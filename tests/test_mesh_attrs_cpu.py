"""CPU checks of the intrinsic mesh export (include/oi_mesh_attr.h, oi_amd.mesh.vertex_attributes / save_ply,
oi_amd.inference.export_mesh): the PLY layouts, the argument checks of Python and of the C ABI, header <=> library <=>
binding, the coverage rule for the new header, and the REHEARSAL of the vertex pass on the fp64 oracle
(tests/helpers/mesh_attr_ref.py) that fixes what the GPU tests may expect of the safeguards.

Rehearsal results (oracle alone, float64, golden weights, bounds [-1, 1]^3, refine = 2; R = 128 is too slow to repeat in
every run and was evaluated once with the same helper):

    R    seeds    threshold   V              flagged  faces disagreeing / judged   residual median per step       worst after
    48   0, 1     0, 0.05     2238 .. 2874   0        0 / 4383 .. 5640             4e-4 .. 6e-4 -> 1e-6 -> 6e-12  1.8e-5
    64   0, 1, 2  0, 0.05     4024 .. 5278   0        0 / 7915 .. 10376            3e-4 -> 4e-7 -> 6e-13          6.3e-6
    128  0, 1, 2  0           20640 .. 21382 0        0 / 40508 .. 42021           6e-5 .. 8e-5 -> 3e-8 -> 3e-15  1.5e-8
    128  0        0.05        16772          0        0 / 32962                    8e-5 -> 2e-8 -> 1e-15          2.2e-9

No vertex comes closer to the half-cell limit than 0.13 of a cell (limit 0.5), the smallest |d sdf/dx| on any mesh is 0.31:
the caps of tests/test_gpu_mesh_attrs.py are therefore ZERO flagged vertices and ZERO disagreeing faces."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import mesh_attr_ref as A

GPU_TEST = os.path.join(ROOT, "tests", "test_gpu_mesh_attrs.py")
KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)

# a two-triangle mesh (a unit square)
V2 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.5]], dtype=np.float64)
T2 = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)


def test_save_ply_without_attributes_is_the_documented_layout_byte_for_byte(tmp_path):
    """The layout the function had before it learnt attributes: the header below, float32 x y z per vertex, then per face one
    uchar 3 and three little-endian int32."""
    from oi_amd import mesh
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            "element face 2\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    body = V2.astype("<f4").tobytes()
    faces = b"".join(b"\x03" + np.asarray(t, dtype="<i4").tobytes() for t in T2)
    expected = head + body + faces
    assert len(expected) == len(head) + 4 * 12 + 2 * 13
    for kw in ({}, dict(normals=None, colors=None)):
        p = tmp_path / "plain.ply"
        mesh.save_ply(str(p), V2, T2, **kw)
        assert p.read_bytes() == expected
    mesh.save_ply(str(p), torch.from_numpy(V2), torch.from_numpy(T2).int())   # tensors are accepted as arrays are
    assert p.read_bytes() == expected


def test_attribute_ply_round_trip(tmp_path):
    from oi_amd import mesh
    rs = np.random.RandomState(0)
    n = A.unit(rs.randn(4, 3)).astype(np.float32)
    c = np.array([[0.0, 1.0, 0.5], [1.5, -0.2, 0.25], [0.1, 0.2, 0.3], [1 / 255, 0.5 / 255, 254.5 / 255]], dtype=np.float32)
    q = np.rint(np.clip(c, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    assert q[0].tolist() == [0, 255, 128] and q[1].tolist() == [255, 0, 64]   # clamp, round half to even
    p = str(tmp_path / "attr.ply")
    mesh.save_ply(p, V2, T2, normals=n, colors=c)
    v, t, props = A.read_ply(p)
    assert props == [("x", "float"), ("y", "float"), ("z", "float"), ("nx", "float"), ("ny", "float"), ("nz", "float"),
                     ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]
    assert v.dtype.itemsize == 27 and np.array_equal(t, T2)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], -1), V2.astype(np.float32))
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], -1), n)
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], -1), q)
    whole = open(p, "rb").read()
    # the interleaved record, as the device writes it, gives the same file; uint8 colours are taken as they are
    rec = np.empty(4, dtype=A.RECORD_DTYPE)
    rec["p"], rec["n"], rec["c"] = V2, n, q
    assert A.RECORD_DTYPE.itemsize == 27 == mesh.RECORD_DTYPE.itemsize
    for verts in (rec.view(np.uint8).reshape(4, 27), torch.from_numpy(rec.view(np.uint8).reshape(4, 27).copy())):
        mesh.save_ply(p, verts, T2)
        assert open(p, "rb").read() == whole
    mesh.save_ply(p, V2, T2, normals=n, colors=q)
    assert open(p, "rb").read() == whole
    # one attribute alone
    mesh.save_ply(p, V2, T2, colors=c)
    v, _, props = A.read_ply(p)
    assert [n_ for n_, _ in props] == ["x", "y", "z", "red", "green", "blue"] and v.dtype.itemsize == 15
    mesh.save_ply(p, V2, T2, normals=n)
    assert [n_ for n_, _ in A.read_ply(p)[2]] == ["x", "y", "z", "nx", "ny", "nz"]
    # an empty mesh
    mesh.save_ply(p, np.zeros((0, 27), dtype=np.uint8), np.zeros((0, 3), dtype=np.int32))
    v, t, _ = A.read_ply(p)
    assert len(v) == 0 and len(t) == 0


def test_python_argument_checks():
    from oi_amd import mesh
    from oi_amd.fields import ShapeNetwork, ColorNetwork, FieldPack
    with pytest.raises(ValueError, match="4 vertices but 3 rows of normals"):
        mesh.save_ply(os.devnull, V2, T2, normals=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="4 vertices but 5 rows of colors"):
        mesh.save_ply(os.devnull, V2, T2, colors=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="already holds"):
        mesh.save_ply(os.devnull, np.zeros((4, 27), dtype=np.uint8), T2, normals=np.zeros((4, 3)))
    net = ShapeNetwork(None, **KW)
    pack = FieldPack(net, ColorNetwork(**KW))
    vi = torch.zeros(5, 3)
    z = torch.zeros(1, 64)
    for bad in (-1, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="refine"):
            mesh.vertex_attributes(pack, vi, (-1,) * 3, (1,) * 3, 16, z=z, refine=bad)
        with pytest.raises(ValueError, match="refine"):
            mesh.extract_intrinsic_mesh(pack, z=z, resolution=16, refine=bad)
    for fn in (lambda o: mesh.vertex_attributes(o, vi, (-1,) * 3, (1,) * 3, 16, z=z),
               lambda o: mesh.extract_intrinsic_mesh(o, z=z, resolution=16)):
        with pytest.raises(ValueError, match="colour head"):
            fn(net)                       # a bare ShapeNetwork
        with pytest.raises(ValueError, match="colour head"):
            fn(FieldPack(net, None))
        with pytest.raises(TypeError):
            fn(object())
    with pytest.raises(ValueError, match="latent"):
        mesh.vertex_attributes(pack, vi, (-1,) * 3, (1,) * 3, 16)
    with pytest.raises(ValueError, match="latent"):
        mesh.extract_intrinsic_mesh(pack, resolution=16)
    with pytest.raises(ValueError, match=r"\(V, 3\)"):
        mesh.vertex_attributes(pack, torch.zeros(5, 2), (-1,) * 3, (1,) * 3, 16, z=z)
    from oi_amd import lib
    with pytest.raises(lib.OiHipError):   # no CPU path
        mesh.vertex_attributes(pack, vi, (-1,) * 3, (1,) * 3, 16, z=z)
    with pytest.raises(ValueError, match="one latent"):
        mesh.extract_intrinsic_mesh(pack, z=torch.zeros(2, 64), resolution=16)


def _header_exports():
    return list(cabi.parse(cabi.read("oi_mesh_attr.h"))[0])


_lib = cabi.built_lib


def test_library_exports_every_mesh_attr_symbol():
    lib, L = _lib()
    names, _ = cabi.check_header("oi_mesh_attr.h", lib)
    assert sorted(names) == ["oi_mesh_attr_finalize", "oi_mesh_newton", "oi_mesh_vertex_record", "oi_mesh_vertex_world"]
    text = cabi.read("oi_mesh_attr.h")
    for macro, val in (("OI_MESH_FLAG_NONFINITE", lib.MESH_FLAG_NONFINITE), ("OI_MESH_FLAG_SMALL_GRADIENT", lib.MESH_FLAG_SMALL_GRADIENT),
                       ("OI_MESH_FLAG_LIMIT", lib.MESH_FLAG_LIMIT), ("OI_MESH_MAX_REFINE", lib.MESH_MAX_REFINE),
                       ("OI_MESH_RECORD_BYTES", lib.MESH_RECORD_BYTES)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == val, macro
    assert (A.FLAG_NONFINITE, A.FLAG_SMALL_GRADIENT, A.FLAG_LIMIT) == (1, 2, 4) and lib.MESH_RECORD_BYTES == A.RECORD_DTYPE.itemsize
    assert float(re.search(r"#define OI_MESH_GRAD_EPS ([0-9.e+-]+)f", text).group(1)) == A.GRAD_EPS
    # the build script compiles the new source
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"mesh_attr.hip"' in src


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x1002)
    world = lambda V=5, xs=f, nx=8, vi=f, pos=f: L.oi_mesh_vertex_world(vi, V, xs, f, f, nx, 8, 8, pos, f, None)
    newton = lambda V=5, pos=f, flags=f, th=0.0, lx=0.1: L.oi_mesh_newton(pos, f, f, f, V, th, lx, 0.1, 0.1, f, flags, None)
    fin = lambda V=5, grad=f, rec=None, sdf=f, res=None, pos=f: L.oi_mesh_attr_finalize(pos, sdf, grad, f, V, 0.0, f, f, res, rec, None)
    rec = lambda V=5, pos=f, r=f: L.oi_mesh_vertex_record(pos, f, f, V, r, None)
    cases = [(lambda: world(V=-1), "oi_mesh_vertex_world", "V=-1"), (lambda: world(V=1 << 31), "oi_mesh_vertex_world", "V=2147483648"),
             (lambda: world(nx=1), "oi_mesh_vertex_world", "lattice 1 x 8 x 8"), (lambda: world(xs=None), "oi_mesh_vertex_world", "null"),
             (lambda: world(pos=None), "oi_mesh_vertex_world", "null"), (lambda: world(vi=None), "oi_mesh_vertex_world", "null"),
             (lambda: newton(V=-3), "oi_mesh_newton", "V=-3"), (lambda: newton(V=1 << 31), "oi_mesh_newton", "V="),
             (lambda: newton(pos=None), "oi_mesh_newton", "null"), (lambda: newton(flags=None), "oi_mesh_newton", "null"),
             (lambda: newton(th=float("nan")), "oi_mesh_newton", "threshold"), (lambda: newton(lx=-0.5), "oi_mesh_newton", "limits"),
             (lambda: fin(V=-1), "oi_mesh_attr_finalize", "V=-1"), (lambda: fin(grad=None), "oi_mesh_attr_finalize", "null"),
             (lambda: fin(rec=odd), "oi_mesh_attr_finalize", "aligned"), (lambda: fin(sdf=None, res=f), "oi_mesh_attr_finalize", "null"),
             (lambda: fin(rec=f, pos=None), "oi_mesh_attr_finalize", "null"),
             (lambda: rec(V=1 << 31), "oi_mesh_vertex_record", "V="), (lambda: rec(pos=None), "oi_mesh_vertex_record", "null"),
             (lambda: rec(r=None), "oi_mesh_vertex_record", "null"), (lambda: rec(r=odd), "oi_mesh_vertex_record", "aligned")]
    for call, entry, text in cases:
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)
    # V = 0: success, nothing launched (null buffers are fine)
    assert L.oi_mesh_vertex_world(None, 0, f, f, f, 8, 8, 8, None, None, None) == 0
    assert L.oi_mesh_newton(None, None, None, None, 0, 0.0, 0.1, 0.1, 0.1, None, None, None) == 0
    assert L.oi_mesh_attr_finalize(None, None, None, None, 0, 0.0, None, None, None, None, None) == 0
    assert L.oi_mesh_vertex_record(None, None, None, 0, None, None) == 0


def _code_only(path):
    import io
    import tokenize
    with open(path) as fh:
        toks = [t for t in tokenize.generate_tokens(io.StringIO(fh.read()).readline)
                if t.type not in (tokenize.COMMENT, tokenize.STRING)]
    return " ".join(t.string for t in toks)


def test_every_mesh_attr_export_has_a_guarded_case():
    """test_bounds_coverage_cpu.py's rule for include/oi_hip.h, applied to include/oi_mesh_attr.h: every entry is called
    through the C ABI on GuardSet buffers by tests/test_gpu_mesh_attrs.py::test_guarded_shapes."""
    src = _code_only(GPU_TEST)
    tree = ast.parse(open(GPU_TEST).read())
    guarded = next(ast.get_source_segment(open(GPU_TEST).read(), n) for n in tree.body
                   if isinstance(n, ast.FunctionDef) and n.name == "_guarded_pass")
    assert 'pytest.mark.usefixtures("guarded_ops")' in open(GPU_TEST).read()
    for n in _header_exports():
        assert re.search(r"\. %s \(" % n, src), f"{n}: no case of tests/test_gpu_mesh_attrs.py calls it"
        assert re.search(r"\.%s\(" % n, guarded), f"{n}: not called on guarded buffers"
    assert "torch.empty" not in guarded and "torch.zeros" not in guarded


def test_newton_rule_safeguards_in_the_restatement():
    lim = np.array([0.1, 0.2, 0.3])
    p0 = np.zeros((6, 3))
    p = p0.copy()
    s = np.array([0.05, 0.05, np.nan, 0.05, 0.5, -0.05])
    g = np.array([[1, 0, 0], [0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [1, 0, 0], [0, 0, 0.5]], dtype=np.float64)
    q, res, f = A.newton_step(p, p0, s, g, lim)
    assert f.tolist() == [0, A.FLAG_SMALL_GRADIENT, A.FLAG_NONFINITE, A.FLAG_NONFINITE, A.FLAG_LIMIT, 0]
    assert np.array_equal(q[[1, 2, 3, 4]], p[[1, 2, 3, 4]])                       # flagged vertices stay
    assert np.allclose(q[0], [-0.05, 0, 0]) and np.allclose(q[5], [0, 0, 0.1])    # p - s g / |g|^2
    assert res[0] == 0.05 and np.isinf(res[1]) and np.isnan(res[2]) and res[4] == 0.5 and res[5] == 0.1
    # index -> world: exact on lattice planes, and the last plane does not look past the axis
    ax = A.axes((-1, -1, -1), (1, 1, 1), (5, 4, 3))
    vw = A.vertex_world(np.array([[4, 0, 2], [1.25, 3, 0], [0, 2.5, 1]]), ax)
    assert np.array_equal(vw[0], [ax[0][4], ax[1][0], ax[2][2]])
    assert vw[1, 0] == ax[0][1] + 0.25 * (ax[0][2] - ax[0][1]) and vw[2, 1] == ax[1][2] + 0.5 * (ax[1][3] - ax[1][2])


@pytest.mark.parametrize("seed,R,threshold", [(0, 64, 0.0), (1, 64, 0.0), (2, 64, 0.0), (0, 64, 0.05), (1, 48, 0.05)])
def test_rehearsal_on_the_oracle_has_no_flagged_vertex_and_no_disagreeing_face(seed, R, threshold):
    """The caps of the GPU tests: the reference itself, in float64, flags nothing and winds every judged face with its normals,
    before and after the refinement; two steps take every vertex inside the sdf parity bar."""
    r = A.rehearsal(seed, R, threshold, refine=2)
    print(r)
    assert r["V"] > 2000 and r["F"] > 4000
    assert r["flagged"] == 0 and r["flag_bits"] == 0
    assert r["faces_judged"] > 0.95 * r["F"]
    assert r["faces_disagree"] == 0 and r["faces_disagree_refine0"] == 0
    assert r["max_shift_cells"] < 0.25          # nowhere near the half-cell limit
    med, worst = r["residual_median"], r["residual_max"]
    assert med[2] < med[1] < med[0] and worst[2] < 1e-4 < worst[0]
