"""Generates object-intrinsics_amd/csrc/mc_tables.h, the marching-cubes case table of csrc/mesh.hip.

    python tools/gen_mc_tables.py            # rewrite the header
    python tools/gen_mc_tables.py --check    # exit 1 if the committed header differs

The table is derived from one rule instead of being typed in (a hand-typed 256 x 16 table cannot be reviewed, and the
classic Lorensen / Bourke table leaves cracks at ambiguous faces):

  * corner c = x + 2 y + 4 z of the cell; a corner is INSIDE iff u > threshold; an edge CROSSES iff its ends differ.
  * edge 4 a + k runs along axis a (0 x, 1 y, 2 z) from the corner with bit a clear and the other two bits k (lower axis
    first) to that corner with bit a set -- the edge lattice point (cell origin + those two bits) owns as its +a edge.
  * face rule: on each of the 6 faces the crossing points are joined pairwise -- two crossings: one segment; four
    (diagonal inside corners, the ambiguous face): two segments that CUT OFF EACH INSIDE CORNER.  The rule reads only the
    face's four corners, so two cells that share a face draw the same segments and the mesh is crack-free by construction.
  * every crossing edge lies on two faces, so the segments form disjoint cycles; each is oriented counter-clockwise seen
    from the outside (u <= threshold) and fan-triangulated from its lowest-numbered edge -- or from the first vertex after
    it whose fan draws no diagonal across a face (fan_apex).  The normal (v1-v0) x (v2-v0)
    then points towards lower u (out of the object for u = -sdf), and a closed mesh has positive signed volume.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "object-intrinsics_amd", "csrc", "mc_tables.h")


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def _edges():
    """edge id -> (axis, start corner, end corner)."""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for k in range(4):
            s = ((k & 1) << b) | ((k >> 1) << c)
            out.append((a, s, s | (1 << a)))
    return out


EDGES = _edges()


def edge_of(c0, c1):
    for e, (_, s, t) in enumerate(EDGES):
        if {s, t} == {c0, c1}:
            return e
    raise KeyError((c0, c1))


def _faces():
    """(axis, side, corners in cyclic order, outward normal) for the 6 faces."""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for s in (0, 1):
            base = s << a
            ring = [base, base | (1 << b), base | (1 << b) | (1 << c), base | (1 << c)]
            n = np.zeros(3)
            n[a] = 1.0 if s else -1.0
            out.append((a, s, ring, n))
    return out


FACES = _faces()


def face_segments(inside, face):
    """The face rule on `face` for corner states `inside` (8 bools): a list of (p, q, m) -- an undirected segment between
    the crossing points of edges p and q, and m, the in-face direction from its inside corner(s) towards the outside."""
    _, _, ring, _ = face
    ins = [inside[c] for c in ring]
    cross = [i for i in range(4) if ins[i] != ins[(i + 1) % 4]]  # ring side i joins ring[i] and ring[i + 1]
    side = lambda i: edge_of(ring[i], ring[(i + 1) % 4])
    if len(cross) == 2:
        pin = np.mean([corner_pos(c) for c, v in zip(ring, ins) if v], axis=0)
        pout = np.mean([corner_pos(c) for c, v in zip(ring, ins) if not v], axis=0)
        return [(side(cross[0]), side(cross[1]), pout - pin)]
    if len(cross) == 4:  # ambiguous: diagonal inside corners, each cut off by its own segment
        centre = np.mean([corner_pos(c) for c in ring], axis=0)
        return [(side((i + 3) % 4), side(i), centre - corner_pos(ring[i])) for i in range(4) if ins[i]]
    return []


def _mid(e):
    _, s, t = EDGES[e]
    return 0.5 * (corner_pos(s) + corner_pos(t))


def directed_face_segments(inside, face):
    """The face's segments oriented so that the cycles they form run counter-clockwise seen from the outside: with m the
    in-face direction towards the outside corners and n the face's outward normal, a segment runs along m x n (the
    polygon then lies inside the cube, on the left of its boundary seen from the tip of the surface normal)."""
    n = face[3]
    out = []
    for p, q, m in face_segments(inside, face):
        d = np.cross(m, n)
        out.append((p, q) if np.dot(_mid(q) - _mid(p), d) > 0 else (q, p))
    return out


def case_polygons(case):
    """The oriented cycles (lists of edge ids, each starting at its lowest-numbered edge) of one case."""
    inside = [bool((case >> c) & 1) for c in range(8)]
    nxt = {}
    for f in FACES:
        for p, q in directed_face_segments(inside, f):
            assert p not in nxt, (case, p)
            nxt[p] = q
    assert sorted(nxt) == sorted(nxt.values()), case  # every crossing edge: one segment in, one out
    cycles, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        cyc = [e]
        seen.add(e)
        while nxt[cyc[-1]] != e:
            cyc.append(nxt[cyc[-1]])
            seen.add(cyc[-1])
        cycles.append(cyc)
    return cycles


def edge_faces(e):
    """The two faces (indices into FACES) edge e lies on."""
    _, s, t = EDGES[e]
    return {f for f, (a, side, ring, _) in enumerate(FACES) if s in ring and t in ring}


def fan_apex(cyc):
    """Position of the fan's apex in the cycle: the first vertex, from the lowest-numbered edge on in cycle order, whose
    fan draws no diagonal between two crossing points of ONE face.  Such a diagonal can only run across an ambiguous face
    whose four crossings lie on one cycle; the neighbour across that face may draw the same one, and the mesh edge would
    then have four triangles instead of two."""
    k = len(cyc)
    for r in range(k):
        if all(not (edge_faces(cyc[r]) & edge_faces(cyc[(r + i) % k])) for i in range(2, k - 1)):
            return r
    raise AssertionError(f"no fan apex for cycle {cyc}")


def case_triangles(case):
    tris = []
    for cyc in case_polygons(case):
        r = fan_apex(cyc)
        c = cyc[r:] + cyc[:r]
        for i in range(1, len(c) - 1):
            tris.append((c[0], c[i], c[i + 1]))
    return tris


def tables():
    """-> (max triangles per case, list of 256 triangle lists)."""
    tri = [case_triangles(c) for c in range(256)]
    return max(len(t) for t in tri), tri


def render():
    mx, tri = tables()
    L = ["// generated by tools/gen_mc_tables.py -- do not edit; rerun the generator instead.",
         "// Marching-cubes case table (rule: tools/gen_mc_tables.py; DESIGN section 4.10).  Corner c = x + 2y + 4z of the cell;",
         "// case bit c set iff corner c is inside (u > threshold).  Edge 4a + k runs along axis a from the corner with bit a",
         "// clear and the other two bits k (lower axis first).  Row: triangles as edge-id triples, counter-clockwise seen from",
         "// the outside, padded with -1.",
         "// (device constant memory: HIP only)",
         "#pragma once",
         "",
         f"#define MC_MAX_TRIS {mx}",
         "",
         "// edge -> (axis, start corner)",
         "static __constant__ const signed char mc_edge_axis[12] = {" + ", ".join(str(a) for a, _, _ in EDGES) + "};",
         "static __constant__ const signed char mc_edge_corner[12] = {" + ", ".join(str(s) for _, s, _ in EDGES) + "};",
         "",
         "static __constant__ const unsigned char mc_tri_count[256] = {"]
    cnt = [len(t) for t in tri]
    for r in range(0, 256, 32):
        L.append("    " + ", ".join(str(c) for c in cnt[r:r + 32]) + ",")
    L.append("};")
    L.append("")
    L.append("static __constant__ const signed char mc_tri_table[256][MC_MAX_TRIS * 3] = {")
    for c in range(256):
        row = [e for t in tri[c] for e in t] + [-1] * (3 * (mx - len(tri[c])))
        L.append("    {" + ", ".join(str(e) for e in row) + "},  // " + str(c))
    L.append("};")
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("mc_tables.h up to date" if same else "mc_tables.h differs from the generator's output")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as fh:
        fh.write(text)
    print(HEADER)
