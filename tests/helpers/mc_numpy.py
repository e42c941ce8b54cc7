"""Numpy restatement of the marching cubes of csrc/mesh.hip, from the generator's table
(tools/gen_mc_tables.py) and the same output order:

  vertices  one per crossing lattice edge, ordered by the owning point's linear index (z fastest), then axis x, y, z;
            in index space: the point plus t = (iso - u0) / (u1 - u0) along the axis, in float32 as the kernel does;
  triangles ordered by the cell's linear index (= its origin point's), then table order; vertex ids shared per edge.
"""
import os
import sys

import numpy as np

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import gen_mc_tables as G  # noqa: E402

MAX_TRIS, _TRIS = G.tables()
TRI_COUNT = np.array([len(t) for t in _TRIS], dtype=np.int64)
TRI_TABLE = np.full((256, MAX_TRIS * 3), -1, dtype=np.int64)
for _c, _t in enumerate(_TRIS):
    TRI_TABLE[_c, :3 * len(_t)] = np.array(_t, dtype=np.int64).reshape(-1)
EDGE_AXIS = np.array([a for a, _, _ in G.EDGES], dtype=np.int64)
EDGE_CORNER = np.array([s for _, s, _ in G.EDGES], dtype=np.int64)


def marching_cubes(u, iso):
    """-> (V,3) float32 index-space vertices, (F,3) int64 triangles."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    iso = np.float32(iso)
    nx, ny, nz = u.shape
    strides = np.array([ny * nz, nz, 1], dtype=np.int64)
    inside = u > iso
    cross = np.zeros(u.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    slot = np.flatnonzero(cross.reshape(-1))  # point * 3 + axis, ascending = the kernel's order
    p, a = slot // 3, slot % 3
    uf = u.reshape(-1)
    u0, u1 = uf[p], uf[p + strides[a]]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (iso - u0) / (u1 - u0)
    verts = np.stack(np.unravel_index(p, u.shape), axis=1).astype(np.float32)
    rows = np.arange(len(p))
    verts[rows, a] = verts[rows, a] + t
    ids = np.full(uf.size * 3, -1, dtype=np.int64)
    ids[slot] = rows

    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.nonzero(TRI_COUNT[case])  # lexicographic = the cells' linear order
    cc = case[ci, cj, ck]
    origin = ci * strides[0] + cj * strides[1] + ck
    n = TRI_COUNT[cc]
    cell = np.repeat(np.arange(len(cc)), n)
    k = np.arange(len(cell)) - np.repeat(np.cumsum(n) - n, n)  # triangle number inside its cell
    edges = TRI_TABLE[cc[cell][:, None], 3 * k[:, None] + np.arange(3)[None, :]]
    corner = EDGE_CORNER[edges]
    pt = origin[cell][:, None] + (corner & 1) * strides[0] + ((corner >> 1) & 1) * strides[1] + (corner >> 2)
    tris = ids[pt * 3 + EDGE_AXIS[edges]]
    return verts, tris.reshape(-1, 3)


def directed_edges_balanced(tris):
    """True iff every directed edge (a, b) of the mesh has exactly one reverse (b, a) and occurs once: a closed, consistently
    wound 2-manifold edge structure."""
    tris = np.asarray(tris, dtype=np.int64)
    if len(tris) == 0:
        return True
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    n = int(e.max()) + 1
    key = e[:, 0] * n + e[:, 1]
    rev = e[:, 1] * n + e[:, 0]
    if len(np.unique(key)) != len(key):
        return False
    return bool(np.array_equal(np.sort(key), np.sort(rev)))


def signed_volume(verts, tris):
    v = np.asarray(verts, dtype=np.float64)[np.asarray(tris, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)
