"""CPU checks of mesh extraction: the generated marching-cubes table (tools/gen_mc_tables.py -> csrc/mc_tables.h), its
numpy restatement (tests/helpers/mc_numpy.py) on analytic and noise fields, save_ply, and the argument checks of
NeuSRenderer.extract_geometry that fail before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_mc_tables as G  # noqa: E402
from helpers import mc_numpy as M  # noqa: E402

R = 24


def _grid():
    g = np.arange(R, dtype=np.float64)
    return np.meshgrid(g, g, g, indexing="ij")


def sphere_field(radius=9.0):
    X, Y, Z = _grid()
    c = (R - 1) / 2
    return (radius - np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2)).astype(np.float32), c, radius


def torus_field():
    X, Y, Z = _grid()
    c = (R - 1) / 2
    q = np.sqrt((X - c) ** 2 + (Y - c) ** 2) - 6.0
    return (2.5 - np.sqrt(q ** 2 + (Z - c) ** 2)).astype(np.float32)


def noise_field(seed=0):
    """Seeded noise, dense in ambiguous faces; the outer two layers are outside so the surface stays off the boundary."""
    u = np.random.default_rng(seed).standard_normal((R, R, R)).astype(np.float32)
    u[:2], u[-2:], u[:, :2], u[:, -2:], u[:, :, :2], u[:, :, -2:] = -1, -1, -1, -1, -1, -1
    return u


def test_generator_reproduces_committed_header():
    with open(G.HEADER) as fh:
        assert fh.read() == G.render()


def test_table_rows_sized_from_max_triangle_count():
    mx, tri = G.tables()
    assert mx == max(len(t) for t in tri)
    assert f"#define MC_MAX_TRIS {mx}" in G.render()
    assert len(tri[0]) == 0 and len(tri[255]) == 0


def _crossing_edges(case):
    ins = [(case >> c) & 1 for c in range(8)]
    return {e for e, (_, s, t) in enumerate(G.EDGES) if ins[s] != ins[t]}


@pytest.mark.parametrize("case", range(256))
def test_case_uses_exactly_the_crossing_edges(case):
    used = {e for t in G.case_triangles(case) for e in t}
    assert used == _crossing_edges(case)


@pytest.mark.parametrize("case", range(256))
def test_case_boundary_on_each_face_is_the_face_rule(case):
    """Polygon edges (not fan diagonals) between crossing points of one face = the face rule's segments on that face."""
    inside = [bool((case >> c) & 1) for c in range(8)]
    segs = {frozenset((a, b)) for cyc in G.case_polygons(case) for a, b in zip(cyc, cyc[1:] + cyc[:1])}
    for f, face in enumerate(G.FACES):
        on_face = {s for s in segs if all(f in G.edge_faces(e) for e in s)}
        rule = {frozenset((p, q)) for p, q, _ in G.face_segments(inside, face)}
        assert on_face == rule, (case, f)
    # and every mesh edge inside the cell that joins two points of one face is such a segment (no fan diagonal across a face)
    for t in G.case_triangles(case):
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            if G.edge_faces(a) & G.edge_faces(b):
                assert frozenset((a, b)) in segs, (case, t)


@pytest.mark.parametrize("case", range(256))
def test_case_directed_edges_pair_inside_cell(case):
    """Each directed interior edge of a cell's triangles has exactly one reverse; boundary edges appear once."""
    from collections import Counter
    d = Counter()
    for t in G.case_triangles(case):
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            d[(a, b)] += 1
    assert all(v == 1 for v in d.values())
    segs = {(a, b) for cyc in G.case_polygons(case) for a, b in zip(cyc, cyc[1:] + cyc[:1])}
    for (a, b) in d:
        if (a, b) not in segs:
            assert d[(b, a)] == 1, (case, a, b)


def test_case_winding_points_to_lower_u():
    """Single inside corner 0: the normal (v1 - v0) x (v2 - v0) points away from it (towards the outside, lower u)."""
    (e0, e1, e2), = G.case_triangles(1)
    v = [G._mid(e) for e in (e0, e1, e2)]
    n = np.cross(v[1] - v[0], v[2] - v[0])
    assert np.dot(n, np.mean(v, axis=0) - G.corner_pos(0)) > 0


@pytest.mark.parametrize("name", ["sphere", "torus", "noise0", "noise1", "noise2"])
def test_numpy_mesh_watertight_and_positive_volume(name):
    u = {"sphere": lambda: sphere_field()[0], "torus": torus_field, "noise0": lambda: noise_field(0),
         "noise1": lambda: noise_field(1), "noise2": lambda: noise_field(2)}[name]()
    v, t = M.marching_cubes(u, 0.0)
    assert len(t) > 100
    assert M.directed_edges_balanced(t)
    assert M.signed_volume(v, t) > 0
    assert np.array_equal(np.unique(t), np.arange(len(v)))  # every vertex is used


def test_numpy_sphere_vertices_on_the_radius():
    u, c, r = sphere_field()
    v, t = M.marching_cubes(u, 0.0)
    err = np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - r)
    # linear interpolation of a distance field along a lattice edge leaves the chord's sag, up to about d^2 / (2 r) for a
    # crossing d off the edge's closest approach: 1.3 % of a voxel at worst for r = 9, the largest radius that keeps the
    # sphere off the boundary of a 24^3 box -- so the mean is held to 1 % and the maximum to 2 %
    assert err.mean() < 0.01 and err.max() < 0.02, (err.mean(), err.max())
    vol = M.signed_volume(v, t)
    assert abs(vol - 4 / 3 * np.pi * r ** 3) < 0.02 * vol


def _read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    v = np.frombuffer(data, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    f = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + 12 * nv)
    assert (f["n"] == 3).all() and end + 12 * nv + 13 * nf == len(data)
    return v, f["i"]


def test_save_ply_round_trip(tmp_path):
    from oi_amd import mesh
    v, t = M.marching_cubes(torus_field(), 0.0)
    p = tmp_path / "torus.ply"
    mesh.save_ply(str(p), v.astype(np.float64), t)
    v2, t2 = _read_ply(str(p))
    assert np.array_equal(v2, v.astype(np.float32)) and np.array_equal(t2, t)


def _renderer():
    from oi_amd.fields import ShapeNetwork, ColorNetwork, SingleVarianceNetwork
    from oi_amd.renderer import NeuSRenderer
    kw = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
    return NeuSRenderer(None, ShapeNetwork(None, **kw), SingleVarianceNetwork(0.3), ColorNetwork(**kw), 16, 16, 0, 1, 0)


def test_extract_geometry_argument_checks():
    r = _renderer()
    b0, b1 = torch.tensor([-1.0, -1, -1]), torch.tensor([1.0, 1, 1])
    with pytest.raises(NotImplementedError):
        r.extract_geometry(b0, b1, 16, siren_network=object(), z=torch.zeros(1, 64))
    with pytest.raises(ValueError):
        r.extract_geometry(b0, b1, 16)
    with pytest.raises(ValueError):
        r.extract_geometry(b0, b1, 16, z=torch.zeros(2, 64))
