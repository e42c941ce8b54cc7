"""CPU restatement of the anti-aliasing stage of the traced renderer (include/oi_aa.h), which touches no
code under test:

    classify     the three criteria in numpy fp32, every product and sum rounded on its own and associated as the header
                 states them, so the flagged set is the kernel's bit for bit
    sub_rays     the sub-pixel pixel coordinates and camera rays in float64
    resolve      the mean over a flagged pixel's samples in numpy fp32, summed in ascending sample order, one division
    r2_pattern   the default pattern

plus the synthetic surfaces (one per criterion) that the CPU test and the GPU test both classify."""
import numpy as np

HIT = 1                                                  # OI_TRACE_HIT
MAX_SAMPLES, DEFAULT_PLANE, DEFAULT_COS = 64, 0.5, 0.5   # OI_AA_*
R2 = (0.7548776662466927, 0.5698402909980532)
f32 = np.float32


def r2_pattern(S):
    """offsets[j] = frac(0.5 + j R2) - 0.5 in float64, rounded to float32.  -> (S, 2)."""
    v = 0.5 + np.arange(S, dtype=np.float64)[:, None] * np.asarray(R2, dtype=np.float64)[None, :]
    return (v - np.floor(v) - 0.5).astype(np.float32)


def _dot(a, b):
    """(a . b) over the last axis in fp32: (x + y) + z, each product rounded."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def classify(status, hit_slot, hit_points, grad, H, W, plane=DEFAULT_PLANE, cos=DEFAULT_COS, parts=False):
    """-> flagged (H * W,) bool.  parts: -> (mask, plane, normal) criteria separately, each (H * W,) bool."""
    status, hit_slot = np.asarray(status).reshape(H, W), np.asarray(hit_slot).reshape(H, W).astype(np.int64)
    n_hit = len(hit_points)
    hit = (status == HIT) & (hit_slot >= 0) & (hit_slot < n_hit)
    k = np.where(hit, hit_slot, 0)
    pts = np.zeros((H, W, 3), f32)
    g = np.zeros((H, W, 3), f32)
    if n_hit:
        pts, g = np.asarray(hit_points, f32)[k], np.asarray(grad, f32)[k]
    gg = _dot(g, g)
    s2, c2 = f32(plane) * f32(plane), f32(cos) * f32(cos)
    out = [np.zeros((H, W), bool) for _ in range(3)]

    def window(a, dy, dx):
        """(a at p, a at q = p + (dy, dx)) over the pixels p whose neighbour q lies inside the image."""
        ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
        yq, xq = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
        return a[ys, xs], a[yq, xq], (ys, xs)

    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy == 0 and dx == 0:
                    continue
                hp, hq, at = window(hit, dy, dx)
                xp, xq, _ = window(pts, dy, dx)
                gp, gq, _ = window(g, dy, dx)
                gpp, gqq, _ = window(gg, dy, dx)
                both = hp & hq
                u = xq - xp
                uu = _dot(u, u)
                dp, dq = _dot(gp, u), _dot(gq, u)
                off = (dp * dp > (s2 * gpp) * uu) | (dq * dq > (s2 * gqq) * uu)
                d = _dot(gp, gq)
                turned = (d <= 0) | (d * d < (c2 * gpp) * gqq)
                out[0][at] |= hp != hq
                out[1][at] |= both & off
                out[2][at] |= both & turned
    out = [o.reshape(-1) for o in out]
    return tuple(out) if parts else out[0] | out[1] | out[2]


def sub_rays(c2b, kinv, offs, R, pixels, offsets):
    """The sub-pixel rays of `pixels` (flagged pixel e = y * R + x) at offsets (S, 2), float64: ray (j - 1) * n + e is sample j
    in 1 .. S - 1.  -> rays_o, rays_d ((S - 1) n, 3), near, far."""
    M, Ki, offs = np.asarray(c2b, np.float64).reshape(4, 4), np.asarray(kinv, np.float64).reshape(3, 3), np.asarray(offs, np.float64)
    pixels, offsets = np.asarray(pixels, np.int64), np.asarray(offsets, np.float64)
    S, n = len(offsets), len(pixels)
    pitch = R / (R - 1.0)
    x, y = pixels % R, pixels // R
    px = (x * pitch + offs[0])[None, :] + offsets[1:, 0, None] * pitch
    py = (y * pitch + offs[1])[None, :] + offsets[1:, 1, None] * pitch
    p = np.stack([px, py, np.ones_like(px)], -1).reshape(-1, 3) @ Ki.T
    p /= np.linalg.norm(p, axis=-1, keepdims=True)
    d = p @ M[:3, :3].T
    o = np.broadcast_to(M[:3, 3], d.shape).copy()
    mid = -(o * d).sum(-1) / (d * d).sum(-1)
    assert d.shape == ((S - 1) * n, 3)
    return o, d, mid - 1.0, mid + 1.0


def resolve(centre, sub, edge_slot, S):
    """centre (P, N), sub (P, (S - 1) n_edge), edge_slot (N,) -> (P, N) fp32: centre off the flagged pixels, elsewhere
    (centre + sub_1 + ... + sub_{S-1}) / S summed in ascending order."""
    centre, edge_slot = np.asarray(centre, f32), np.asarray(edge_slot, np.int64)
    out = centre.copy()
    on = np.nonzero(edge_slot >= 0)[0]
    if len(on) == 0:
        return out
    sub = np.asarray(sub, f32)
    n_edge = sub.shape[1] // (S - 1)
    acc = centre[:, on]
    for j in range(1, S):
        acc = acc + sub[:, (j - 1) * n_edge + edge_slot[on]]
    out[:, on] = acc / f32(S)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# synthetic surfaces: every pixel hits (so the mask criterion is silent), one case per criterion
# ---------------------------------------------------------------------------------------------------------------------
SYN_H, SYN_W, SYN_PITCH = 6, 8, 0.05      # pixel (x, y) looks down -z at (x, y) * SYN_PITCH; the step / crease runs along x = 3.5


def _case(z, normal):
    H, W = SYN_H, SYN_W
    ys, xs = np.mgrid[0:H, 0:W]
    pts = np.stack([xs * SYN_PITCH, ys * SYN_PITCH, np.broadcast_to(z, (H, W))], -1).reshape(-1, 3).astype(f32)
    grad = (np.broadcast_to(normal, (H, W, 3)).reshape(-1, 3) * 1.7).astype(f32)     # the raw gradient: not unit
    perm = np.random.RandomState(3).permutation(H * W)                                 # hits are listed in no fixed order
    slot = np.empty(H * W, np.int32)
    slot[perm] = np.arange(H * W, dtype=np.int32)
    return dict(status=np.full(H * W, HIT, np.uint8), hit_slot=slot, hit_points=pts[perm], grad=grad[perm], H=H, W=W)


def synthetic(name):
    """'plane': a tilted plane (nothing to flag).  'step': a depth step of 0.4 seen face-on.  'grazing_step': the same jump
    whose near side is grazing -- a steep wall that contains the jump direction, so its normal is perpendicular to the jump
    and only the far side's normal sees it.  'crease90' / 'crease30': two planes that meet between the columns 3 and 4 with
    normals 90 / 30 degrees apart, continuous in depth.
    -> (the arrays classify takes, the columns x that must be flagged -- all others must not be)"""
    H, W = SYN_H, SYN_W
    x = np.arange(W)[None, :] * SYN_PITCH
    left = np.arange(W)[None, :] < W // 2
    edge = (W // 2 - 1, W // 2)
    up = np.array([0.0, 0.0, 1.0])
    if name == "plane":
        n = np.array([0.3, 0.0, 1.0]) / np.linalg.norm([0.3, 0.0, 1.0])
        return _case(-n[0] / n[2] * x, n), ()
    if name == "step":
        return _case(np.where(left, 0.0, -0.4), up), edge
    if name == "grazing_step":
        n_near = np.array([0.4, 0.0, SYN_PITCH]) / np.linalg.norm([0.4, 0.0, SYN_PITCH])   # perpendicular to (pitch, 0, -0.4)
        x_rim = (W // 2 - 1) * SYN_PITCH
        z_near = -(x - x_rim) * n_near[0] / n_near[2]                                   # the wall through the rim (x_rim, ., 0)
        return _case(np.where(left, z_near, -0.4), np.where(left[..., None], n_near, up)), edge
    if name in ("crease90", "crease30"):
        half = np.deg2rad(45.0 if name == "crease90" else 15.0)
        nl, nr = np.array([-np.sin(half), 0.0, np.cos(half)]), np.array([np.sin(half), 0.0, np.cos(half)])
        xc = (W // 2 - 0.5) * SYN_PITCH
        return _case(-np.abs(x - xc) * np.tan(half), np.where(left[..., None], nl, nr)), (edge if name == "crease90" else ())
    raise KeyError(name)


SYNTHETIC = ("plane", "step", "grazing_step", "crease90", "crease30")
