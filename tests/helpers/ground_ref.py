"""float64 numpy restatement of include/oi_ground.h, built from the existing restatements: the scene's
rays, transform and cull of helpers.scene_ref, the sample numbers and directions of helpers.occlusion_ref, the aimed sample and
the local lights' factors of helpers.local_light_ref, "missed every instance" of helpers.scene_light_ref.  It covers the pixel
classification, the construction of the ground points' secondary rays in every element (fed the kernel's own float32
directions for the cull, as scene_light_ref.rays is), the resolve over chunks, the shade with its matte, and the occlude rule --
plus the closed forms of the analytic two-sphere scene on a ground plane.  Nothing here touches the code under test."""
import numpy as np

from helpers import local_light_ref as LL
from helpers import occlusion_ref as R
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T

MISS, HIT, BACKFACING, MARCH = T.MISS, T.HIT, T.BACKFACING, T.MARCH
FLOATS = 12                          # OI_GROUND_FLOATS
FRONT = 1e-6                         # n . d < -FRONT: the front face
SEED = SL.SEED

# the analytic scene's plane (tests/test_ground_cpu.py rehearses the conditions on float64 alone): "up" is -y in the world of
# the example camera, the plane lies 0.1 below sphere 0 and is a disc of radius 4 about the origin
AN_NORMAL, AN_OFFSET, AN_EXTENT, AN_CENTRE = (0.0, -1.0, 0.0), -0.6, 4.0, (0.0, 0.0, 0.0)
AN_GROUND_LIGHT = (0.3, -1.0, -0.4)  # from the ground TO the light
AN_AO_S, AN_AO_DISTANCE = 4, 2.0
AN_CUT_OFFSET = -0.2                 # the plane n . x = -0.2 passes through sphere 0: it hides the part of it below
# bands of the analytic comparisons: float32 may decide either way inside them
ND_BAND, RIM_BAND = 1e-5, 1e-4


def record(normal, offset, albedo=(0.8, 0.8, 0.8), extent=np.inf, centre=(0.0, 0.0, 0.0)):
    """The 12 floats, as the header lays them out."""
    return np.array([*normal, offset, *albedo, extent, *centre, 0.0], dtype=np.float64)


def analytic_record(offset=AN_OFFSET):
    return record(AN_NORMAL, offset, (0.7, 0.6, 0.5), AN_EXTENT, AN_CENTRE)


# ---------------------------------------------------------------------------------------------------------------------
# classification
# ---------------------------------------------------------------------------------------------------------------------
def classify(c2w, K_inv, S, rec, owner=None, t_owner=None):
    """oi_ground_begin.  owner (S * S,) int (-1: none) and t_owner (S * S,) the owner's ray parameter, or None: nothing is
    owned.  -> dict: ground (S * S,) bool, t (NaN off the ground), p (S * S, 3), nd, rim = |p - c| - R_g, o (3,), d (S * S, 3),
    front (the plane is met in front, within the extent, whatever owns the pixel)."""
    rec = np.asarray(rec, dtype=np.float64)
    n, h, Rg, c = rec[:3], rec[3], rec[7], rec[8:11]
    o, d = SR.scene_rays(c2w, K_inv, S)
    d = d.reshape(-1, 3)
    nd = d @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (h - n @ o) / nd
        p = o + t[:, None] * d
        rim = np.linalg.norm(p - c, axis=-1) - Rg
    front = (nd < -FRONT) & (t > 0) & (rim <= 0)
    ground = front.copy()
    if owner is not None:
        owned = np.asarray(owner) >= 0
        ground &= ~owned | (t < np.where(owned, np.asarray(t_owner, dtype=np.float64), np.inf))   # a tie goes to the instance
    return dict(ground=ground, t=np.where(ground, t, np.nan), t_all=t, p=p, nd=nd, rim=rim, o=o, d=d, front=front)


RAY_EPS = 16                         # float32 make_ray: a direction component is within 16 eps of the float64 one (t_bar)


def t_bar(o, d, rec):
    """The float32 rounding bar of t_g = (h - n . o) / (n . d), every product and sum rounded once, on the float32 ray of
    make_ray: its origin is a copy of c2w's column (exact); a component of its direction carries the rounding of the pixel
    coordinate (1 eps), the 3 x 3 product with K^-1 (3), the normalisation (3 products, 2 sums, a root, a quotient: 5) and the
    3 x 3 product with the pose (3), 12 eps of a value <= 1, taken as RAY_EPS = 16.  The numerator's error is at most eps (3
    sum |n_i o_i| + |h - n . o|), the denominator's eps (3 sum |n_i d_i| + 16 sum |n_i|), the quotient adds eps |t|.  The
    denominator's error enters as |t| / |n . d|: the bar scales with 1 / |n . d|.  1.01 covers the higher orders.  -> (S * S,)."""
    eps = 2.0 ** -24
    rec = np.asarray(rec, dtype=np.float64)
    n, h = rec[:3], rec[3]
    nd = d @ n
    num = h - n @ o
    e_num = eps * (3 * np.abs(n * o).sum() + abs(num))
    e_den = eps * (3 * (np.abs(d) * np.abs(n)).sum(-1) + RAY_EPS * np.abs(n).sum())
    t = num / nd
    return 1.01 * (e_num / np.abs(nd) + np.abs(t) * e_den / np.abs(nd) + eps * np.abs(t))


# ---------------------------------------------------------------------------------------------------------------------
# the ground points' secondary rays
# ---------------------------------------------------------------------------------------------------------------------
def world_directions(rec, pixel, seed, S, j0, Sc, light_dirs=None, radius=None, origins=None, local=None):
    """The directions of samples j0 .. j0 + Sc - 1 of S, drawn in the WORLD frame.  pixel (n,).  light_dirs (L, 3) + radius (L,):
    the caps -> d (L, Sc, n, 3); neither: the cosine hemisphere about n -> (1, Sc, n, 3); local (L, 20) + origins (n, 3): aimed at
    the local lights -> d (L, Sc, n, 3), and t_light (L, Sc, n), inside (L, n).  -> dict d, t_light, inside."""
    n3 = np.asarray(rec, dtype=np.float64)[:3]
    nrm = np.broadcast_to(n3, (len(pixel), 3))
    if local is not None:
        d, tl, ins = [], [], []
        for lt in np.asarray(local, dtype=np.float64).reshape(-1, LL.FLOATS):
            q, rad = LL.in_frame(lt, np.eye(4))
            a = LL.aimed(origins, nrm, pixel, q, rad, S, seed, j0, Sc)
            d.append(np.where(a["inside"][None, :, None], 0.0, a["d"]))
            tl.append(a["t_light"])
            ins.append(a["inside"])
        return dict(d=np.stack(d), t_light=np.stack(tl), inside=np.stack(ins))
    if light_dirs is None:
        d = SL.owner_directions(nrm, pixel, seed, S, j0, Sc)
    else:
        axes = np.stack([np.broadcast_to(T.light_object_dir(l, np.eye(4)), (len(pixel), 3)) for l in light_dirs])
        d = SL.owner_directions(nrm, pixel, seed, S, j0, Sc, axes, radius)
    return dict(d=d, t_light=None, inside=None)


def rays(rec, p, pixel, w2b, bias, S, j0, Sc, seed, light_dirs=None, radius=None, distance=None, local=None, d_world=None):
    """oi_ground_rays_begin.  p (n, 3) the ground points, pixel (n,), w2b (E, 4, 4).  One of: light_dirs (L, 3) + radius (L,);
    distance (the hemisphere); local (L, 20).  d_world (L, Sc, n, 3): directions to use instead of drawing them (the kernel's
    own, to restate the rest of the construction on its inputs).
    -> dict: d_world (L, Sc, n, 3); per element o, d (E, L, Sc, n, 3), near, far, c2 (E, L, Sc, n), status (E, L, Sc, n) with MARCH
    for an entered ray; traced (L, Sc, n); limit (L, Sc, n) (inf: none)."""
    rec, w2b = np.asarray(rec, dtype=np.float64), np.asarray(w2b, dtype=np.float64)
    n3 = rec[:3]
    o_world = np.asarray(p, dtype=np.float64) + bias * n3
    drawn = world_directions(rec, pixel, seed, S, j0, Sc, light_dirs, radius, o_world, local)
    if d_world is None:
        d_world = drawn["d"]
    d_world = np.asarray(d_world, dtype=np.float64)
    L, n, E = d_world.shape[0], len(pixel), len(w2b)
    limit = np.full((L, Sc, n), np.inf)
    inside = np.zeros((L, 1, n), dtype=bool)
    if local is not None:
        limit, inside = drawn["t_light"], drawn["inside"][:, None]
    elif light_dirs is None:
        limit = np.full((L, Sc, n), float(distance))
    facing = (d_world @ n3) > 0
    traced = facing & ~inside
    shape = (E, L, Sc, n)
    o, d = np.zeros(shape + (3,)), np.zeros(shape + (3,))
    near, far, c2 = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    status = np.zeros(shape, dtype=np.uint8)
    for e in range(E):
        o[e] = np.broadcast_to(SR.transform(w2b[e], o_world), (L, Sc, n, 3))
        d[e] = np.einsum("ab,lsnb->lsna", w2b[e][:3, :3], d_world)
        with np.errstate(divide="ignore", invalid="ignore"):     # (a ray whose origin is inside a light has no direction)
            ent, ne, fa, c2[e] = SR.cull(o[e], d[e])
        ent = ent & (ne < limit) & traced
        near[e], far[e] = np.where(ent, ne, 0.0), np.where(ent, np.minimum(fa, limit), 0.0)
        status[e] = np.where(np.broadcast_to(inside, traced.shape), MISS, np.where(facing, np.where(ent, MARCH, MISS), BACKFACING))
    return dict(d_world=d_world, o=o, d=d, near=near, far=far, c2=c2, status=status, traced=traced, limit=limit)


def counts(chunks, S):
    """oi_ground_resolve over the chunks' finished states, each (E, L, Sc, n_g), in order.  -> count (L, n_g) int, out (L, n_g):
    count / S in float32."""
    count = sum(SL.escaped(st).sum(1) for st in chunks).astype(np.int64)
    return count, (count.astype(np.float32) / np.float32(S)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# shade
# ---------------------------------------------------------------------------------------------------------------------
def shade(rec, p, lights, local=False, visibility=None, ao=None):
    """oi_ground_shade at the ground points p (n, 3).  lights (L, 16) directional or (L, 20) local, world frame; visibility (L,
    n), ao (n,) or None.  -> image, matte (L, 3, n), and the rounding bars of both (L, 3, n) for a float32 evaluation that rounds
    every product, sum and quotient once, fed these very points (shade_bar)."""
    rec, p = np.asarray(rec, dtype=np.float64), np.asarray(p, dtype=np.float64)
    n3, alb = rec[:3], rec[4:7]
    nn = len(p)
    aov = np.ones(nn) if ao is None else np.asarray(ao, dtype=np.float64)
    image, matte, bar_i, bar_m = [], [], [], []
    for li, lt in enumerate(np.asarray(lights, dtype=np.float64).reshape(-1, LL.FLOATS if local else 16)):
        if local:
            l, att, spot = LL.factors(p, lt, np.eye(4))
            slope = 0.0 if lt[11] <= -1 else 1.5 / (lt[19] - lt[11])
        else:
            l, att, spot, slope = np.broadcast_to(T.light_object_dir(lt[:3], np.eye(4)), (nn, 3)), np.ones(nn), np.ones(nn), 0.0
        k0 = att * spot
        rl = np.maximum(l @ n3, 0.0)
        vis = np.ones(nn) if visibility is None else np.asarray(visibility, dtype=np.float64)[li]
        dk = lt[8:11][:, None] * (rl * k0)[None]
        value = (lt[4:7][:, None] * aov[None] + dk * vis[None]) * alb[:, None]
        full = (lt[4:7][:, None] + dk) * alb[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(full == 0, 1.0, value / full)
        bv, bf = (shade_bar(lt, alb, n3, l, att, spot, slope, a, v, local) for a, v in ((aov, vis), (np.ones(nn), np.ones(nn))))
        with np.errstate(divide="ignore", invalid="ignore"):
            bm = np.where(full == 0, 0.0, (bv + np.abs(m) * bf) / np.abs(full) + 2.0 ** -24 * np.abs(m))
        image.append(value), matte.append(m), bar_i.append(bv), bar_m.append(bm)
    return np.stack(image), np.stack(matte), np.stack(bar_i), np.stack(bar_m)


def shade_bar(lt, alb, n3, l, att, spot, slope, ao, vis, local):
    """The float32 rounding bar (3, n) of (ambient ao + diffuse max(n . l, 0) k0 vis) albedo, eps = 2^-24.  The ambient term
    passes 3 roundings (its product, the sum, the albedo).  The diffuse term passes 5 (three products, the sum, the albedo)
    and carries the error of max(n . l, 0): 3 eps sum |n_i l_i| of the rounded dot product and the error of l -- directional:
    the quotient by |l| and the normalisation, 8 eps per component; local: the difference q - p, its norm and the quotient,
    6 eps -- so (3 + 8) eps sum |n_i l_i|.  Local lights add the error of att (the difference, three products and two sums, d0^2,
    the max, the quotient: 10 eps att) and of spot = smoothstep(tt), |d spot / d tt| <= 1.5, tt = (c - cos_outer) / (cos_inner -
    cos_outer) with c = -(l . a): l's 6 eps, the axis's normalisation 6 eps, the dot product 3 eps, the quotient and the
    polynomial 10 eps of a value <= 1: 1.5 * 15 eps / (cos_inner - cos_outer) + 10 eps, absolute.  1.01 covers the higher orders."""
    eps = 2.0 ** -24
    nl = (np.abs(l) * np.abs(n3)).sum(-1)
    amb = np.abs(lt[4:7])[:, None] * ao[None]
    dif = np.abs(lt[8:11])[:, None]
    rl = np.maximum(l @ n3, 0.0)
    e = 3 * amb + dif * (5 * rl + 11 * nl)[None] * (att * spot * vis)[None]
    if local:
        e = e + dif * (rl * vis * (10 * att * spot + att * (slope * 15 + 10)))[None]
    return 1.01 * eps * e * alb[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# the ground as occluder
# ---------------------------------------------------------------------------------------------------------------------
def occlude(status, o, d, elem, b2w, rec, limit):
    """oi_ground_occlude.  status (E, Q) uint8, o, d (E, Q, 3) the chunk's rays (box frames), elem (n_vis,), Q a multiple of
    n_vis, b2w (E, 4, 4).  -> the new status (E, Q); t (Q,) the plane's ray parameter on the owner's ray; rim (Q,)."""
    rec, b2w = np.asarray(rec, dtype=np.float64), np.asarray(b2w, dtype=np.float64)
    n3, h, Rg, c = rec[:3], rec[3], rec[7], rec[8:11]
    Q = status.shape[1]
    own = np.asarray(elem)[np.arange(Q) % len(elem)]
    ob, db = np.asarray(o, dtype=np.float64)[own, np.arange(Q)], np.asarray(d, dtype=np.float64)[own, np.arange(Q)]
    ow = np.einsum("qab,qb->qa", b2w[own][:, :3, :3], ob) + b2w[own][:, :3, 3]
    dw = np.einsum("qab,qb->qa", b2w[own][:, :3, :3], db)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (h - ow @ n3) / (dw @ n3)
        rim = np.linalg.norm(ow + t[:, None] * dw - c, axis=-1) - Rg
    hit = (t > 0) & (t < limit) & (rim <= 0)
    out = np.array(status, copy=True)
    was = out[own, np.arange(Q)]
    out[own, np.arange(Q)] = np.where((was == MISS) & hit, HIT, was)
    return out, t, rim


# ---------------------------------------------------------------------------------------------------------------------
# the analytic two-sphere scene on the plane
# ---------------------------------------------------------------------------------------------------------------------
def analytic_ground(sc, cf, rec):
    """The analytic scene's ground in float64: classify() against the closed form's owner and depth."""
    return classify(sc["c2w"], sc["K_inv"], sc["S"], rec, cf["owner"], np.where(cf["owner"] >= 0, cf["depth"], np.inf))


def analytic_shadows(g, light=AN_GROUND_LIGHT, bias=T.BIAS, rec=None):
    """The hard shadows of the two spheres on the ground points: -> q (the ground pixels), blocked (2, n), band (2, n), lit (n,)."""
    rec = analytic_record() if rec is None else rec
    q = np.nonzero(g["ground"])[0]
    l = np.asarray(light, dtype=np.float64) / np.linalg.norm(light)
    o = g["p"][q] + bias * np.asarray(rec[:3])
    blocked, band = SL.sphere_blocks(o, np.broadcast_to(l, o.shape))
    return dict(q=q, blocked=blocked, band=band, lit=~blocked.any(0))
