"""float64 numpy restatement of the scene layer (include/oi_scene.h): the scene's rays, the bounding-
sphere cull, the windows, the depth resolve across instances with its tie rule, the visible lists and their prefix offsets,
the combination of the shadow states, the world transform -- and the closed forms of the analytic two-sphere scene.  Plus
the poses and shapes the CPU and GPU tests share.  Nothing here touches the code under test."""
import numpy as np

import oi_oracle as O
from helpers import trace_ref as T

MISS, HIT, BACKFACING = T.MISS, T.HIT, T.BACKFACING
MAX_ELEMS = 1024


# ---------------------------------------------------------------------------------------------------------------------
# camera and rays
# ---------------------------------------------------------------------------------------------------------------------
def camera(R):
    """The example camera of a generator of crop resolution R: (S, K (3, 3), K_inv (3, 3), c2w, w2c (4, 4)), float64, from the
    oracle's float32 matrices (what the library's camera buffers hold)."""
    cam_dist, scene_fov, S = T.example_camera(R)
    K, K_inv, c2w, w2c = O.camera_matrices(cam_dist, scene_fov, S)
    f = lambda m: m.double().numpy()
    return S, f(K)[:3, :3], f(K_inv)[:3, :3], f(c2w), f(w2c)


def rigid_inverse(m):
    m = np.asarray(m, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = m[:3, :3].T
    out[:3, 3] = -m[:3, :3].T @ m[:3, 3]
    return out


def pixel_coords(S):
    """linspace(0, 1, S) * S: the coordinate of scene pixel X (not X)."""
    return np.linspace(0.0, 1.0, S) * S


def scene_rays(c2b, K_inv, S):
    """-> o (3,), d (S, S, 3) [Y][X] of the scene's rays in the frame c2b maps the camera to."""
    c = pixel_coords(S)
    px, py = np.meshgrid(c, c, indexing="xy")
    p = np.stack([px, py, np.ones_like(px)], -1) @ np.asarray(K_inv, dtype=np.float64).T
    v = p / np.linalg.norm(p, axis=-1, keepdims=True)
    c2b = np.asarray(c2b, dtype=np.float64)
    return c2b[:3, 3].copy(), v @ c2b[:3, :3].T


def cull(o, d):
    """The unit sphere's chord on rays (o, d) (any leading shape): -> entered (bool), near, far, c2, with mid = -o.d / d.d,
    c2 = |o + mid d|^2, h = sqrt((1 - c2) / d.d); entered: c2 < 1 and mid + h > 0; near = max(mid - h, 0), far = mid + h
    (both 0 where not entered)."""
    o, d = np.broadcast_arrays(np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64))
    dd, od = (d * d).sum(-1), (o * d).sum(-1)
    mid = -od / dd
    c = o + mid[..., None] * d
    c2 = (c * c).sum(-1)
    h = np.sqrt(np.maximum(1.0 - c2, 0.0) / dd)
    entered = (c2 < 1.0) & (mid + h > 0)
    return entered, np.where(entered, np.maximum(mid - h, 0.0), 0.0), np.where(entered, mid + h, 0.0), c2


def window_pixels(origin, W):
    """Scene pixel (X, Y) of each local ray j * W + i of a window: two (W * W,) int arrays."""
    j, i = np.divmod(np.arange(W * W), W)
    return origin[0] + i, origin[1] + j


def min_window(b2ws, R):
    """Brute force in float64: per instance the bounding box (x_lo, x_hi, y_lo, y_hi) of the scene pixels -- of an image
    extended far beyond S x S -- whose ray passes within 1 of the box origin."""
    S, K, K_inv, c2w, w2c = camera(R)
    out = []
    pad = 4 * S
    c = (np.arange(-pad, S + pad)) * (S / (S - 1))          # linspace's coordinate, continued outside the image
    px, py = np.meshgrid(c, c, indexing="xy")
    p = np.stack([px, py, np.ones_like(px)], -1) @ K_inv.T
    v = p / np.linalg.norm(p, axis=-1, keepdims=True)
    for m in b2ws:
        centre = (w2c @ np.asarray(m, dtype=np.float64))[:3, 3]
        along = v @ centre
        dist2 = centre @ centre - along ** 2
        ys, xs = np.nonzero((dist2 < 1.0) & (along > 0))
        out.append((xs.min() - pad, xs.max() - pad, ys.min() - pad, ys.max() - pad))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# resolve, visible lists, visibility
# ---------------------------------------------------------------------------------------------------------------------
def resolve(status, t, origins, W, S):
    """status, t (E, W * W); origins (E, 2).  -> owner, owner_ray (S * S,) int: the HIT with the smallest t among the
    windows covering a pixel, equal t to the lowest element index; -1 without a hit."""
    owner, owner_ray = np.full(S * S, -1, dtype=np.int64), np.full(S * S, -1, dtype=np.int64)
    best = np.full(S * S, np.inf)
    for e in range(len(status)):
        X, Y = window_pixels(origins[e], W)
        ok = (X >= 0) & (X < S) & (Y >= 0) & (Y < S) & (np.asarray(status[e]) == HIT)
        q, r = (Y * S + X)[ok], np.arange(W * W)[ok]
        better = (owner[q] < 0) | (np.asarray(t[e], dtype=np.float64)[r] < best[q])      # strict: a tie keeps the earlier element
        owner[q[better]], owner_ray[q[better]], best[q[better]] = e, r[better], np.asarray(t[e], dtype=np.float64)[r[better]]
    return owner, owner_ray


def visible_sets(owner, owner_ray, E):
    """Per element the sorted local rays that own their pixel."""
    return [np.sort(owner_ray[owner == e]) for e in range(E)]


def offsets(counts):
    """Exclusive prefix sum."""
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


def combine_visibility(shadow_status, owner, owner_ray, vis_slot, offset):
    """shadow_status (E, L, n_vis); vis_slot (E, N).  -> (L, S * S): 1 off the mask, on it 1 only where the pixel's ray ended
    MISS in every element."""
    E, L, _ = shadow_status.shape
    vis = np.ones((L, len(owner)))
    on = np.nonzero(owner >= 0)[0]
    g = offset[owner[on]] + vis_slot[owner[on], owner_ray[on]]
    vis[:, on] = (shadow_status[:, :, g] == MISS).all(0)
    return vis


def transform(m, p):
    """The 4 x 4 rigid m applied to points p (n, 3), float64."""
    m = np.asarray(m, dtype=np.float64)
    return np.asarray(p, dtype=np.float64) @ m[:3, :3].T + m[:3, 3]


def transform_bar(m, p):
    """The float32 rounding bar of one component of m p computed as three products and three sums (any order of the sums):
    each product is rounded once and takes part in at most three rounded sums, the translation in at most three: |error| <=
    4 u sum_k |m_ak p_k| + 3 u |m_a3| to first order, u = 2^-24; 1.01 covers the higher orders.  -> (n, 3)."""
    m, p = np.abs(np.asarray(m, dtype=np.float64)), np.abs(np.asarray(p, dtype=np.float64))
    return 1.01 * 2.0 ** -24 * (4 * (p @ m[:3, :3].T) + 3 * m[:3, 3])


# ---------------------------------------------------------------------------------------------------------------------
# the test scenes on the golden field
# ---------------------------------------------------------------------------------------------------------------------
def shifted(name, dx=0.0, dy=0.0, dz=0.0):
    """The test pose `name` (helpers.trace_ref.pose) moved by (dx, dy, dz) in the world."""
    m = T.pose(name).clone()
    m[0, 3] += dx
    m[1, 3] += dy
    m[2, 3] += dz
    return m


def scene_poses(kind):
    """(seed, pose) per instance.  'pair': two instances that overlap in the image, the second nearer the camera; 'triple':
    the pair and an instance on the image's edge, whose window lies half outside the image; 'twice': one instance entered twice at one pose;
    'offscreen': the pair's first instance and one far outside the image; 'single': one instance."""
    near = shifted("centre", 0.55, -0.35, -1.6)
    return {"pair": [(0, T.pose("centre")), (1, near)],
            "triple": [(0, T.pose("centre")), (1, near), (2, shifted("off", -0.42, 0.0, 0.0))],
            "twice": [(1, T.pose("centre")), (1, T.pose("centre"))],
            "offscreen": [(0, T.pose("centre")), (1, shifted("centre", 40.0, 0.0, 0.0))],
            "single": [(2, shifted("centre", -0.4, 0.3, 0.0))],
            "nothing": [(0, shifted("centre", 40.0, 0.0, 0.0)), (1, shifted("centre", 0.0, -40.0, 0.0))]}[kind]


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene: two spheres of radius 0.5, each the field |x| - 0.5 in its own box frame
# ---------------------------------------------------------------------------------------------------------------------
RADIUS = 0.5
AN_S, AN_W, AN_DIST, AN_FOV = 32, 16, 6.0, 24.0
AN_CENTRES = np.array([[0.0, 0.0, 0.0], [0.42, -0.33, -1.05]])
AN_LIGHT = AN_CENTRES[1] - AN_CENTRES[0]              # from the surface TO the light: sphere 1 stands in between
AN_DEPTH_GAP, AN_SILHOUETTE, AN_SHADOW_EDGE, AN_CAP = 1e-4, 1e-3, 1e-3, 0.03
# depth bar of one pixel: the march ends at |sdf| <= tol; the float32 evaluation of |o + t d| - 0.5 at coordinates up to
# AN_DIST + 1 adds 3 roundings of ulp(8) / 2 = 4.8e-7 each in the point and 2 in the norm, < 2e-6; a sdf error e moves t by
# e / cos(incidence)
AN_SDF_SLACK = T.TOL + 2e-6


def analytic_scene():
    """-> dict: S, W, K_inv (3, 3), c2w, b2w (2, 4, 4), c2b (2, 4, 4), origins (2, 2) (windows centred on the spheres'
    projections), light (3,) (world, not normalised)."""
    S = AN_S
    focal = (S / 2) / np.tan(0.5 * AN_FOV * np.pi / 180)
    K = np.array([[focal, 0, 0.5 * S], [0, focal, 0.5 * S], [0, 0, 1.0]])
    c2w = np.eye(4)
    c2w[2, 3] = -AN_DIST
    rot = T.pose("centre").double().numpy()[:3, :3]      # any rotation: the field does not care, the frames do
    b2w = np.stack([np.eye(4), np.eye(4)])
    b2w[0, :3, :3], b2w[1, :3, :3] = rot, rot.T
    b2w[:, :3, 3] = AN_CENTRES
    c2b = np.stack([rigid_inverse(m) @ c2w for m in b2w])
    origins = []
    for c in AN_CENTRES:
        cc = c - c2w[:3, 3]
        pix = (K @ (cc / cc[2]))[:2] * (S - 1) / S
        origins.append(np.round(pix - (AN_W - 1) / 2).astype(np.int64))
    return dict(S=S, W=AN_W, K_inv=np.linalg.inv(K), c2w=c2w, b2w=b2w, c2b=c2b, origins=np.array(origins), light=AN_LIGHT.copy())


def analytic_closed_form(sc):
    """Per scene pixel (S * S,) in float64: owner (-1: none), depth, the exclusion mask of the owner / depth comparison,
    the per-pixel depth bar, and for the pixels sphere 0 owns its visibility with sphere 1 and without, the exclusion mask
    of the shadow comparison and n . l."""
    S = sc["S"]
    o, d = scene_rays(sc["c2w"], sc["K_inv"], S)
    d = d.reshape(-1, 3)
    ts, rho, bars = [], [], []
    for c in AN_CENTRES:
        oc = o - c
        b = d @ oc
        perp2 = oc @ oc - b * b
        disc = RADIUS ** 2 - perp2
        ts.append(np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0.0)), np.inf))
        rho.append(np.sqrt(perp2))
        bars.append(AN_SDF_SLACK / np.sqrt(np.maximum(1.0 - perp2 / RADIUS ** 2, 1e-30)))
    ts, rho, bars = np.array(ts), np.array(rho), np.array(bars)
    owner = np.where(np.isfinite(ts).any(0), ts.argmin(0), -1)
    depth = ts.min(0)
    both = np.isfinite(ts).all(0)
    gap = np.abs(np.where(both, ts[0], 0.0) - np.where(both, ts[1], 0.0))
    excluded = (np.abs(rho - RADIUS) < AN_SILHOUETTE).any(0) | (both & (gap < AN_DEPTH_GAP))
    bar = np.where(owner >= 0, np.take_along_axis(bars, np.maximum(owner, 0)[None], 0)[0], np.inf)
    # shadows on sphere 0
    l = sc["light"] / np.linalg.norm(sc["light"])
    on0 = owner == 0
    p = o + depth[on0, None] * d[on0]
    n = (p - AN_CENTRES[0]) / RADIUS
    ndl = n @ l
    so = p + T.BIAS * n
    along = (AN_CENTRES[1] - so) @ l
    closest = np.linalg.norm(so + np.maximum(along, 0.0)[:, None] * l - AN_CENTRES[1], axis=-1)
    lit_alone = ndl > 0
    lit = lit_alone & ~(closest < RADIUS)
    shadow_excluded = lit_alone & (np.abs(closest - RADIUS) < AN_SHADOW_EDGE)
    return dict(owner=owner, depth=depth, excluded=excluded, bar=bar, gap=np.where(both, gap, np.inf),
                both_bar=bars.sum(0), on0=on0, lit=lit, lit_alone=lit_alone, shadow_excluded=shadow_excluded, ndl=ndl)
