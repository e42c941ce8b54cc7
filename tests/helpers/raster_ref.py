"""Restatement of the mesh rasteriser of include/oi_raster.h: the setup in float64, the coverage rule
in integers, the depth and the attribute lookup in float64 -- and a brute-force float64 ray / triangle caster that knows
nothing of pixels' fixed point.

    camera / rays / project             the GEOMETRY paragraph of the header (csrc/ray_common.h's ray, its inverse)
    snap / classify                     oi_raster_setup, rule by rule
    covers_int / covers                 the top-left rule in Python integers (one centre) and in int64 arrays (a box)
    plane_t / raster                    the depth and the visible triangle: per pixel the two nearest candidates
    cast                                Moeller-Trumbore on every (ray, triangle) pair, no snapping
    barycentric / vertex_attr / texture_attr   oi_raster_resolve's attributes
    icosphere / quad / fan / soup       the meshes the tests share

Nothing here touches the code under test."""
import numpy as np

FIX = 256
MAX_FIX = (1 << 22) * FIX
DROPPED, EMPTY, SMALL, LARGE = 0, 1, 2, 3
EPS32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def camera(R, seed=0, distance=2.5, focal=1.6, offsets=True):
    """A test camera looking at the origin from `distance`: -> dict of c2b, b2c (4, 4), K, kinv (3, 3), offs (2,), float32
    values held as float64 arrays (what the kernels are given, exactly).  The crop offsets shift the window by a fraction of
    a pixel and a few whole pixels so that a wrong sign or scale of them shows."""
    rs = np.random.RandomState(seed)
    z = rs.randn(3)
    z /= np.linalg.norm(z)                          # the viewing direction
    x = np.cross(z, rs.randn(3))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2b = np.eye(4)
    c2b[:3, 0], c2b[:3, 1], c2b[:3, 2], c2b[:3, 3] = x, y, z, -distance * z
    offs = (rs.rand(2) * 2.0 - 1.0) * (1.3 if offsets else 0.0)
    f = focal * R
    K = np.array([[f, 0.0, 0.5 * R + offs[0]], [0.0, f, 0.5 * R + offs[1]], [0.0, 0.0, 1.0]])
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    c2b, K, offs = f32(c2b), f32(K), f32(offs)
    return {"c2b": c2b, "b2c": f32(np.linalg.inv(c2b)), "K": K, "kinv": f32(np.linalg.inv(K)), "offs": offs, "R": R}


def pixel_coord(R, i, off):
    """csrc/ray_common.h's pixel_coord in float64: linspace(0, 1, R)[i] * R + off."""
    return (0.0 if R == 1 else np.asarray(i, dtype=np.float64) / (R - 1)) * R + off


def rays(cam):
    """make_ray for every pixel in float64: -> o (3,), d (R, R, 3) indexed [Y, X]."""
    R = cam["R"]
    X, Y = np.meshgrid(np.arange(R), np.arange(R))
    p = np.stack([pixel_coord(R, X, cam["offs"][0]), pixel_coord(R, Y, cam["offs"][1]), np.ones((R, R))], -1) @ cam["kinv"].T
    p /= np.linalg.norm(p, axis=-1, keepdims=True)
    return cam["c2b"][:3, 3].copy(), p @ cam["c2b"][:3, :3].T


def project(cam, pts):
    """Raster coordinates (n, 2) and camera depth (n,) of box-frame points: pixel centres are the integers."""
    R = cam["R"]
    pc = np.asarray(pts, dtype=np.float64) @ cam["b2c"][:3, :3].T + cam["b2c"][:3, 3]
    q = pc @ cam["K"].T
    scale = (R - 1) / R if R > 1 else 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        xy = (q[:, :2] / pc[:, 2:3] - cam["offs"][None]) * scale
    return xy, pc[:, 2]


# ---------------------------------------------------------------------------------------------------------------------
# setup
# ---------------------------------------------------------------------------------------------------------------------
def snap(xy):
    return np.rint(np.asarray(xy, dtype=np.float64) * FIX)


def orientation(c):
    """Sign of the area of the corners c (3, 2), Python integers."""
    (ax, ay), (bx, by), (cx, cy) = [[int(v) for v in p] for p in c]
    a = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    return (a > 0) - (a < 0)


def classify(corners, ok, R, small_max):
    """corners (F, 3, 2) integers, ok (F,) bool (False: dropped) -> cls (F,) uint8 and bbox (F, 4) of include/oi_raster.h."""
    F = len(corners)
    cls, bbox = np.zeros(F, dtype=np.uint8), np.tile(np.array([0, 0, -1, -1], dtype=np.int64), (F, 1))
    for f in range(F):
        if not ok[f]:
            continue
        c = [[int(v) for v in p] for p in corners[f]]
        xs, ys = [p[0] for p in c], [p[1] for p in c]
        x0, x1 = max(-(-min(xs) // FIX), 0), min(max(xs) // FIX, R - 1)
        y0, y1 = max(-(-min(ys) // FIX), 0), min(max(ys) // FIX, R - 1)
        cls[f] = EMPTY
        if orientation(c) != 0 and x0 <= x1 and y0 <= y1:
            bbox[f] = (x0, y0, x1, y1)
            cls[f] = SMALL if (x1 - x0 + 1) * (y1 - y0 + 1) <= small_max else LARGE
    return cls, bbox


def setup(cam, pos, tris, near, small_max):
    """oi_raster_setup in float64 and integers: -> corners (F, 3, 2) int64 (zeros where dropped), exact projections (F, 3, 2)
    float64 in fixed-point units, cls, bbox."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    xy, depth = project(cam, pos)
    fix = xy * FIX
    s = snap(xy)
    good = (depth > near) & np.isfinite(s).all(1) & (np.abs(s) <= MAX_FIX).all(1)
    ok = good[tris].all(1) if len(tris) else np.zeros(0, dtype=bool)
    corners = np.where(ok[:, None, None], np.nan_to_num(s)[tris], 0).astype(np.int64) if len(tris) else np.zeros((0, 3, 2), np.int64)
    cls, bbox = classify(corners, ok, cam["R"], small_max)
    return corners, fix[tris] if len(tris) else np.zeros((0, 3, 2)), cls, bbox


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
def _edge_in(a, b, px, py):
    dx, dy = b[0] - a[0], b[1] - a[1]
    w = dx * (py - a[1]) - dy * (px - a[0])
    return w > 0 or (w == 0 and (dy < 0 or (dy == 0 and dx > 0)))


def covers_int(c, X, Y):
    """Does the triangle with the snapped corners c (3, 2) cover the centre of pixel (X, Y)?  Python integers throughout."""
    c = [[int(v) for v in p] for p in c]
    o = orientation(c)
    if o == 0:
        return False
    a, b, d = (c[0], c[1], c[2]) if o > 0 else (c[0], c[2], c[1])
    px, py = int(X) * FIX, int(Y) * FIX
    return _edge_in(a, b, px, py) and _edge_in(b, d, px, py) and _edge_in(d, a, px, py)


def covers(c, x0, y0, x1, y1):
    """covers_int over the box x0 .. x1, y0 .. y1 at once in int64 (exact while the coordinates stay below 2^30) -> bool
    (y1 - y0 + 1, x1 - x0 + 1)."""
    c = np.asarray(c, dtype=np.int64)
    assert np.abs(c).max() <= 1 << 30
    o = orientation(c)
    if o == 0:
        return np.zeros((y1 - y0 + 1, x1 - x0 + 1), dtype=bool)
    order = (0, 1, 2) if o > 0 else (0, 2, 1)
    px, py = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64) * FIX, np.arange(y0, y1 + 1, dtype=np.int64) * FIX)
    inside = np.ones(px.shape, dtype=bool)
    for k in range(3):
        a, b = c[order[k]], c[order[(k + 1) % 3]]
        dx, dy = b[0] - a[0], b[1] - a[1]
        w = dx * (py - a[1]) - dy * (px - a[0])
        inside &= (w > 0) | ((w == 0) & bool(dy < 0 or (dy == 0 and dx > 0)))
    return inside


def plane_t(v, o, d):
    """The ray parameter of rays (o, d (..., 3)) on the plane of the triangle v (3, 3), and n . d of the UNIT normal."""
    n = np.cross(v[1] - v[0], v[2] - v[0])
    den = d @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (n @ (v[0] - o)) / den
    nn = np.linalg.norm(n)
    return t, den / nn if nn > 0 else np.zeros_like(den)


def raster(cam, pos, tris, corners, cls, bbox):
    """The visible triangle of every pixel from the SNAPPED corners: -> ids (R, R) int64 (-1 off the mesh), t (R, R) the
    nearest depth (NaN off the mesh), second (R, R) the depth of the nearest OTHER candidate (inf without one), cosine (R, R)
    |n . d| of the visible triangle's unit normal, count (R, R) how many triangles cover the centre.  Equal depths go to the
    lower index."""
    R = cam["R"]
    o, d = rays(cam)
    pos, tris = np.asarray(pos, dtype=np.float64), np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    ids, best = np.full((R, R), -1, dtype=np.int64), np.full((R, R), np.inf)
    second, cosine, count = np.full((R, R), np.inf), np.zeros((R, R)), np.zeros((R, R), dtype=np.int64)
    for f in range(len(tris)):
        if cls[f] not in (SMALL, LARGE):
            continue
        x0, y0, x1, y1 = (int(v) for v in bbox[f])
        cov = covers(corners[f], x0, y0, x1, y1)
        if not cov.any():
            continue
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        t, nd = plane_t(pos[tris[f]], o, d[sl])
        cand = cov & np.isfinite(t) & (t > 0)
        count[sl] += cand
        b, s2 = best[sl], second[sl]
        win = cand & (t < b)            # (strictly: an equal depth stays with the lower index, visited first)
        lose = cand & ~win
        s2[win] = b[win]
        s2[lose] = np.minimum(s2[lose], t[lose])
        b[win] = t[win]
        ids[sl][win] = f
        cosine[sl][win] = np.abs(nd[win])
    return ids, np.where(ids >= 0, best, np.nan), second, cosine, count


def cast(cam, pos, tris):
    """Brute force: the nearest triangle each pixel's ray meets (Moeller-Trumbore, float64, no snapping).  -> ids (R, R),
    t (R, R) (NaN without a hit)."""
    R = cam["R"]
    o, d = rays(cam)
    pos, tris = np.asarray(pos, dtype=np.float64), np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    ids, best = np.full((R, R), -1, dtype=np.int64), np.full((R, R), np.inf)
    for f in range(len(tris)):
        v0, v1, v2 = pos[tris[f]]
        e1, e2 = v1 - v0, v2 - v0
        h = np.cross(d, e2)
        a = h @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (h @ (o - v0)) / a
            q = np.cross(o - v0, e1)
            v = (d @ q) / a
            t = (q @ e2) / a
        hit = (np.abs(a) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < best)
        best[hit] = t[hit]
        ids[hit] = f
    return ids, np.where(ids >= 0, best, np.nan)


def near_edge(cam, fixed, cls, bbox, units=1.0):
    """(R, R) bool: the pixel centres within `units` fixed-point units of an edge of a triangle.  fixed (F, 3, 2): the EXACT projections in fixed-point units.  Only there may a
    rule on snapped corners and the exact geometry disagree."""
    R = cam["R"]
    out = np.zeros((R, R), dtype=bool)
    for f in range(len(fixed)):
        if cls[f] == DROPPED:
            continue
        c = fixed[f]
        x0, x1 = max(int(np.floor(c[:, 0].min() / FIX)) - 1, 0), min(int(np.ceil(c[:, 0].max() / FIX)) + 1, R - 1)
        y0, y1 = max(int(np.floor(c[:, 1].min() / FIX)) - 1, 0), min(int(np.ceil(c[:, 1].max() / FIX)) + 1, R - 1)
        if x0 > x1 or y0 > y1:
            continue
        px, py = np.meshgrid(np.arange(x0, x1 + 1) * float(FIX), np.arange(y0, y1 + 1) * float(FIX))
        for k in range(3):
            a, b = c[k], c[(k + 1) % 3]
            ex, ey = b - a
            l2 = ex * ex + ey * ey
            if l2 > 0:   # the distance to the SEGMENT: the parameter of the foot point clamped to the edge
                s = np.clip(((px - a[0]) * ex + (py - a[1]) * ey) / l2, 0.0, 1.0)
                dist = np.hypot(px - (a[0] + s * ex), py - (a[1] + s * ey))
                out[y0:y1 + 1, x0:x1 + 1] |= dist <= units
    return out


def depth_bar(t, cosine):
    """The bar on a resolved depth: 32 eps t / |n . d| (fp32 eps)."""
    return 32.0 * EPS32 * np.abs(t) / np.maximum(cosine, 1e-30)


# ---------------------------------------------------------------------------------------------------------------------
# attributes
# ---------------------------------------------------------------------------------------------------------------------
def barycentric(v, p):
    """Clamped, renormalised barycentrics (n, 3) of points p (n, 3) on the triangles v (n, 3, 3), from 3-D sub-areas."""
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    sub = lambda a, b: np.einsum("na,na->n", n, np.cross(a - p, b - p))
    b = np.maximum(np.stack([sub(v[:, 1], v[:, 2]), sub(v[:, 2], v[:, 0]), sub(v[:, 0], v[:, 1])], -1), 0.0)
    s = b.sum(-1, keepdims=True)
    return np.where(s > 0, b / np.where(s > 0, s, 1.0), np.array([1.0, 0.0, 0.0]))


def unit(n):
    return n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-6)


def vertex_attr(tri_rows, bary, normals, albedo):
    """Interpolated (unit normal, albedo) (n, 3) each: tri_rows (n, 3) vertex indices, bary (n, 3)."""
    nn = np.einsum("nk,nka->na", bary, np.asarray(normals, dtype=np.float64)[tri_rows])
    return unit(nn), np.einsum("nk,nka->na", bary, np.asarray(albedo, dtype=np.float64)[tri_rows])


def texture_attr(uv_rows, bary, albedo_map, normal_map, sample):
    """The texture mode: uv_rows (n, 3, 2) the corners' coordinates, `sample`: helpers.mesh_tex_ref.sample_bilinear.  Byte
    atlases decode as byte / 255 and byte / 255 * 2 - 1."""
    uv = np.einsum("nk,nka->na", bary, np.asarray(uv_rows, dtype=np.float64))
    a, n = np.asarray(albedo_map), np.asarray(normal_map)
    a = a.astype(np.float64) / 255.0 if a.dtype == np.uint8 else a.astype(np.float64)
    n = n.astype(np.float64) / 255.0 * 2.0 - 1.0 if n.dtype == np.uint8 else n.astype(np.float64)
    return unit(sample(n, uv)), sample(a, uv)


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions=2, radius=0.5):
    """-> pos (V, 3) float32, tris (F, 3) int32, outward orientation: 20 * 4^subdivisions triangles on the sphere."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, dtype=np.int32)


def longest_edge(pos, tris):
    p = np.asarray(pos, dtype=np.float64)[np.asarray(tris, dtype=np.int64)]
    return float(max(np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=-1).max() for k in range(3)))


def quad(flip=False):
    """Two triangles that share the diagonal of a square facing the test camera's origin side; flip: the second triangle in
    the other orientation.  -> pos (4, 3) float32, tris (2, 3) int32."""
    pos = np.array([[-0.4, -0.3, 0.0], [0.45, -0.35, 0.05], [0.4, 0.42, 0.0], [-0.38, 0.4, -0.05]], dtype=np.float32)
    return pos, np.array([[0, 1, 2], [0, 3, 2] if flip else [0, 2, 3]], dtype=np.int32)


def fan(n=7):
    """A closed fan of n triangles about the origin in the plane z = 0.  -> pos (n + 1, 3) float32, tris (n, 3) int32."""
    a = np.arange(n) * 2.0 * np.pi / n + 0.3
    pos = np.concatenate([np.zeros((1, 3)), np.stack([0.45 * np.cos(a), 0.45 * np.sin(a), np.zeros(n)], -1)]).astype(np.float32)
    return pos, np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], dtype=np.int32)


def soup(F=64, seed=0, size=0.5):
    """F random overlapping triangles inside the unit ball.  -> pos (3 F, 3) float32, tris (F, 3) int32."""
    rs = np.random.RandomState(seed)
    centre = rs.rand(F, 1, 3) * 0.8 - 0.4
    pos = (centre + (rs.rand(F, 3, 3) - 0.5) * size).reshape(-1, 3).astype(np.float32)
    return pos, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the cases tests/test_raster_cpu.py rehearses and tests/test_gpu_raster.py runs
# ---------------------------------------------------------------------------------------------------------------------
SPHERE_R, SPHERE_RADIUS, SPHERE_CAM_SEED = 33, 0.5, 3
SOUP_R, SOUP_F, SOUP_SEED, SOUP_CAM_SEED = 33, 64, 1, 1
GRAZING = 0.05      # pixels whose visible triangle has |n . d| below this are excluded from the depth bar


def sphere_case(R=SPHERE_R):
    pos, tris = icosphere(2, SPHERE_RADIUS)
    return camera(R, SPHERE_CAM_SEED), pos, tris


def soup_case():
    pos, tris = soup(SOUP_F, SOUP_SEED)
    return camera(SOUP_R, SOUP_CAM_SEED), pos, tris


def unexamined(t, second, cosine):
    """(R, R) bool: covered pixels whose two nearest candidates lie within the depth bar of each other -- there the fp32 depth
    may order them either way, and the id is not compared."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(t) & (second - t <= 2.0 * depth_bar(t, cosine))


def face_sag(r, h):
    """How deep a triangle inscribed in the sphere of radius r lies under it at the most, given its longest edge h: every
    point of a triangle is within its circumradius of a corner, an acute triangle's circumradius is at most h / sqrt(3) (an
    obtuse one's farthest point is nearer still), so the depth is at most r - sqrt(r^2 - h^2 / 3).  (The sag under the
    midpoint of an EDGE, r - sqrt(r^2 - (h / 2)^2), is smaller: a face's centroid lies deeper than its edges.)"""
    return r - np.sqrt(r * r - h * h / 3.0)


def sphere_gaps(cam, t, r):
    """Of the depth map t (R, R) against the analytic sphere of radius r about the origin: radial (R, R) = r - |o + t d|, how
    deep the point lies under the sphere; along (R, R) = t - t_sphere along the ray; ok (R, R): the ray meets the sphere."""
    o, d = rays(cam)
    b = d @ o
    disc = b * b - (o @ o - r * r)
    ok = disc > 0
    ta = -b - np.sqrt(np.where(ok, disc, 0.0))
    return r - np.linalg.norm(o + t[..., None] * d, axis=-1), t - ta, ok


def along_ray_bound(cam, r, sag):
    """The same bound along the ray: past its entry at t_sphere the ray is at radius^2 = r^2 - 2 c s + s^2 after the length
    s, c = sqrt(disc) the half chord; a point no deeper than `sag` has radius >= r - sag, so
    s <= c - sqrt(c^2 - (2 r sag - sag^2)) -- or, where the ray never gets that deep, the whole chord 2 c."""
    o, d = rays(cam)
    b = d @ o
    c2 = np.maximum(b * b - (o @ o - r * r), 0.0)
    k = 2.0 * r * sag - sag * sag
    return np.where(c2 >= k, np.sqrt(c2) - np.sqrt(np.maximum(c2 - k, 0.0)), 2.0 * np.sqrt(c2))


def tie_square(flip=False):
    """Snapped corners (2, 3, 2) of a square of 8 x 8 pixels whose diagonal runs THROUGH the centres (k, k) and whose outline
    runs through centres too; flip: the second triangle in the other orientation."""
    S = 8 * FIX
    a = [(0, 0), (S, 0), (S, S)]
    b = [(0, 0), (0, S), (S, S)] if flip else [(0, 0), (S, S), (0, S)]
    return np.array([a, b], dtype=np.int64)


def tie_fan():
    """Snapped corners (8, 3, 2) of a closed fan about an apex that IS the centre of pixel (6, 6), rim corners on centres and
    between them, the triangles in mixed orientations; and the rim (8, 2)."""
    apex = (6 * FIX, 6 * FIX)
    rim = [(12 * FIX, 6 * FIX), (10 * FIX + 77, 11 * FIX), (6 * FIX, 12 * FIX), (1 * FIX + 5, 10 * FIX + 130),
           (0, 6 * FIX), (2 * FIX, 1 * FIX), (6 * FIX, 0), (11 * FIX, 2 * FIX + 3)]
    tris = [[apex, rim[k], rim[(k + 1) % 8]] if k % 2 else [apex, rim[(k + 1) % 8], rim[k]] for k in range(8)]
    return np.array(tris, dtype=np.int64), np.array(rim, dtype=np.int64)


def owners(corner_sets, R):
    """(R, R) int64: the triangle whose snapped corners cover each centre by covers_int, -1 for none; asserts that no centre
    is covered twice."""
    out = np.full((R, R), -1, dtype=np.int64)
    for Y in range(R):
        for X in range(R):
            hit = [f for f, c in enumerate(corner_sets) if covers_int(c, X, Y)]
            assert len(hit) <= 1, (X, Y, hit)
            if hit:
                out[Y, X] = hit[0]
    return out
