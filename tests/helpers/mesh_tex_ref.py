"""Restatement of the texture atlas of include/oi_mesh_tex.h in integers and float64, and the
REHEARSAL of the textured export on the fp64 oracle alone (through tests/helpers/mesh_attr_ref.py):

    layout / pixels / corner_uv / barycentrics / points   section "THE ATLAS" of the header, rule by rule
    quant8                                                 the byte of the atlases (the vertex record's rule)
    sample_bilinear / bilinear_taps                        a texture lookup: texel centres at + 0.5, clamp addressing
    refine_with_band                                       the Newton rule with the texels that come near the limit marked
    bake / rehearse_quality / rehearse_band                an atlas built by the oracle, and what the GPU tests may expect

Nothing here touches the code under test."""
import numpy as np

from helpers import mesh_attr_ref as A

MIN_TEXEL, MAX_TEXEL, MAX_SIZE = 3, 64, 16384


def n_texels(T):
    return T * (T + 1) // 2


def layout(F, T):
    """-> (W, H, cols, rows) of the atlas of F triangles at texel size T."""
    assert MIN_TEXEL <= T <= MAX_TEXEL and F >= 0
    ncells = (F + 1) >> 1
    cols = 1
    while cols * cols < ncells:
        cols += 1
    rows = max(1, -(-ncells // cols))
    return cols * (T + 1), rows * T, cols, rows


def texel_ij(T):
    """(n_T,) i and j of the texels k = 0 .. n_T - 1: rows of falling length, k = j T - j (j - 1) / 2 + i."""
    ij = [(i, j) for j in range(T) for i in range(T - j)]
    for k, (i, j) in enumerate(ij):
        assert k == j * T - j * (j - 1) // 2 + i
    a = np.array(ij, dtype=np.int64)
    return a[:, 0], a[:, 1]


def pixels(F, T, f=None):
    """(len(f), n_T, 2) integer pixel (x, y) of every texel of the triangles f (default all F), row 0 on top."""
    _, _, cols, _ = layout(F, T)
    f = np.arange(F, dtype=np.int64) if f is None else np.asarray(f, dtype=np.int64)
    i, j = texel_ij(T)
    c = f >> 1
    x0, y0 = ((c % cols) * (T + 1))[:, None], ((c // cols) * T)[:, None]
    odd = (f & 1).astype(bool)[:, None]
    x = np.where(odd, x0 + T - i[None], x0 + i[None])
    y = np.where(odd, y0 + T - 1 - j[None], y0 + j[None])
    return np.stack([x, y], -1)


def corner_uv(F, T, f=None):
    """(len(f), 3, 2) float64 texture coordinates of the corners: u = x / W, v = 1 - y / H."""
    W, H, cols, _ = layout(F, T)
    f = np.arange(F, dtype=np.int64) if f is None else np.asarray(f, dtype=np.int64)
    c = f >> 1
    x0, y0 = ((c % cols) * (T + 1)).astype(np.float64)[:, None], ((c // cols) * T).astype(np.float64)[:, None]
    cu, cv = np.array([0.0, T - 2.0, 0.0])[None], np.array([0.0, 0.0, T - 2.0])[None]
    odd = (f & 1).astype(bool)[:, None]
    x = np.where(odd, x0 + T + 0.5 - cu, x0 + 0.5 + cu)
    y = np.where(odd, y0 + T - 0.5 - cv, y0 + 0.5 + cv)
    return np.stack([x / W, 1.0 - y / H], -1)


def barycentrics(T):
    """(n_T, 3) float64 (b0, b1, b2) of the texels: b1 = i / (T - 2), b2 = j / (T - 2), b0 = 1 - b1 - b2 (negative in the
    gutter row i + j = T - 1: extrapolated, not clamped)."""
    i, j = texel_ij(T)
    b1, b2 = i / (T - 2.0), j / (T - 2.0)
    return np.stack([1.0 - b1 - b2, b1, b2], -1)


def points(pos, tris, T, f=None):
    """(len(f), n_T, 3) float64 planar points b0 v0 + b1 v1 + b2 v2 of the triangles f (default all)."""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if f is not None:
        t = t[np.asarray(f, dtype=np.int64)]
    v = np.asarray(pos, dtype=np.float64)[t]                      # (n, 3 corners, 3 axes)
    return np.einsum("km,fma->fka", barycentrics(T), v)


def quant8(c):
    """round-to-nearest-even of clamp(c, 0, 1) * 255 in float32, NaN -> 0."""
    c = np.nan_to_num(np.asarray(c, dtype=np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf)
    return np.rint(np.clip(c, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def bilinear_taps(uv, W, H):
    """uv (n, 2) -> taps (n, 4, 2) integer (x, y) BEFORE clamping, and weights (n, 4): texel centres at + 0.5."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    x, y = uv[:, 0] * W - 0.5, (1.0 - uv[:, 1]) * H - 0.5
    xi, yi = np.floor(x), np.floor(y)
    fx, fy = x - xi, y - yi
    xi, yi = xi.astype(np.int64), yi.astype(np.int64)
    taps = np.stack([np.stack([xi, yi], -1), np.stack([xi + 1, yi], -1), np.stack([xi, yi + 1], -1),
                     np.stack([xi + 1, yi + 1], -1)], 1)
    wts = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
    return taps, wts


def sample_bilinear(atlas, uv):
    """Bilinear lookup of an (H, W, C) atlas at uv (n, 2), v up: texel centres at + 0.5, clamp addressing.  float64."""
    a = np.asarray(atlas, dtype=np.float64)
    H, W = a.shape[:2]
    taps, wts = bilinear_taps(uv, W, H)
    tx, ty = np.clip(taps[..., 0], 0, W - 1), np.clip(taps[..., 1], 0, H - 1)
    return (a[ty, tx] * wts[..., None]).sum(1)


def refine_with_band(fn, p0, limit, threshold, refine, rel=1e-4):
    """A.refine_vertices with one more result: near (n,) bool, the points whose candidate came within `rel` (relative) of the
    limit on some axis in some step -- there the fp32 comparison of the kernel may fall on the other side.
    -> positions, (sdf, grad, albedo) there, last residual, flags, near."""
    p, flags = p0.copy(), np.zeros(len(p0), dtype=np.uint8)
    near = np.zeros(len(p0), dtype=bool)
    for _ in range(refine):
        s, g, _ = fn(p)
        g2 = (g * g).sum(-1)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            cand = p - ((s + threshold) / np.maximum(g2, A.GRAD_EPS))[:, None] * g
            near |= (np.abs(np.abs(cand - p0) - limit[None]) <= rel * limit[None]).any(-1)
        p, _, f = A.newton_step(p, p0, s + threshold, g, limit)
        flags |= f
    s, g, c = fn(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = np.abs(s + threshold) / np.sqrt((g * g).sum(-1))
    return p, (s, g, c), res, flags, near


_MESHES = {}


def oracle_mesh(seed, R, threshold=0.0, refine=2):
    """The intrinsic mesh of the oracle in float64 (cached): dict with fn, pos (V, 3), tris (F, 3), albedo (V, 3), limit (3,)."""
    key = (seed, R, threshold, refine)
    if key not in _MESHES:
        import helpers.mc_numpy as M
        import oi_oracle as O
        sd, csd = A.golden_state()
        w = O.style_mlp(sd, A.latent(seed).double())
        ax = A.axes((-1.0,) * 3, (1.0,) * 3, R)
        xx, yy, zz = np.meshgrid(*ax, indexing="ij")
        u = -A.field(sd, None, w, np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1))[0].reshape(xx.shape)
        vi, tris = M.marching_cubes(u, threshold)
        fn = lambda p: A.field(sd, csd, w, p)
        lim = A.half_cell(ax)
        p, (_, _, c), _, _ = A.refine_vertices(fn, A.vertex_world(vi, ax), lim, threshold, refine)
        _MESHES[key] = dict(fn=fn, pos=p, tris=np.asarray(tris, dtype=np.int64), albedo=c, limit=lim)
    return _MESHES[key]


def bake(fn, pos, tris, T, limit, threshold=0.0, refine=2):
    """The float64 albedo atlas (H, W, 3) of a mesh under the oracle `fn`, the flags and the near-limit marks (F, n_T)."""
    F = len(tris)
    W, H, _, _ = layout(F, T)
    p0 = points(pos, tris, T).reshape(-1, 3)
    _, (_, _, c), _, flags, near = refine_with_band(fn, p0, limit, threshold, refine)
    atlas = np.zeros((H, W, 3))
    px = pixels(F, T).reshape(-1, 2)
    atlas[px[:, 1], px[:, 0]] = c
    return atlas, flags.reshape(F, -1), near.reshape(F, -1)


def surface_samples(F, n, seed):
    """n seeded samples on the triangles of a mesh: (triangle index (n,), barycentrics (n, 3) uniform on the triangle)."""
    rs = np.random.RandomState(seed)
    f = rs.randint(0, F, n)
    r1, r2 = np.sqrt(rs.rand(n)), rs.rand(n)
    return f, np.stack([1 - r1, r1 * (1 - r2), r1 * r2], -1)


def quality(fn, pos, tris, vertex_albedo, atlas, T, limit, n=2000, seed=0, threshold=0.0, refine=2):
    """The point of the feature, measured: at n seeded surface samples, the reference is the oracle albedo at the sample's
    oracle Newton projection; (a) the bilinear lookup of `atlas` at the sample's UV, (b) the barycentric interpolation of the
    vertex albedo.  -> (median |a - ref|, median |b - ref|), the error being the largest channel difference per sample."""
    tris = np.asarray(tris, dtype=np.int64)
    f, b = surface_samples(len(tris), n, seed)
    p0 = np.einsum("nm,nma->na", b, np.asarray(pos, dtype=np.float64)[tris[f]])
    _, (_, _, ref), _, _, _ = refine_with_band(fn, p0, limit, threshold, refine)
    uv = np.einsum("nm,nmc->nc", b, corner_uv(len(tris), T, f))
    ea = np.abs(sample_bilinear(atlas, uv) - ref).max(-1)
    eb = np.abs(np.einsum("nm,nmc->nc", b, np.asarray(vertex_albedo, dtype=np.float64)[tris[f]]) - ref).max(-1)
    return float(np.median(ea)), float(np.median(eb))


def rehearse_quality(seed, R, T):
    """-> (median error of the texture, median error of the vertex colours, F) on the oracle alone."""
    m = oracle_mesh(seed, R)
    atlas, _, _ = bake(m["fn"], m["pos"], m["tris"], T, m["limit"])
    ea, eb = quality(m["fn"], m["pos"], m["tris"], m["albedo"], atlas, T, m["limit"])
    return ea, eb, len(m["tris"])


def rehearse_band(seed, R, T, n=20000, sub_seed=0):
    """-> (fraction of a seeded subsample of texels within 1e-4 relative of the limit, fraction flagged) on the oracle."""
    m = oracle_mesh(seed, R)
    p0 = points(m["pos"], m["tris"], T).reshape(-1, 3)
    sel = np.random.RandomState(sub_seed).permutation(len(p0))[:n]
    _, _, _, flags, near = refine_with_band(m["fn"], p0[sel], m["limit"], 0.0, 2)
    return float(near.mean()), float((flags != 0).mean())
