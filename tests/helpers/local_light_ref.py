"""fp64 CPU restatement of include/oi_local_light.h: the local light record, the light in a box frame,
the shadow samples aimed at the light's sphere with the ray's end at the light, the shading with the per-pixel direction, the
inverse-square falloff and the cone, and the scene's rule for an instance that does not own the point -- plus the lights and
settings the CPU rehearsal and the GPU tests share.  Builds on tests/helpers/occlusion_ref.py (sample numbers, tangent frame,
the any-hit machine) and scene_ref.py (the cull); nothing here touches the code under test."""
import numpy as np

from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import scene_ref as SR
from helpers import trace_ref as T

FLOATS = 20                  # OI_LOCAL_LIGHT_FLOATS
MIN_DISTANCE = 1e-3          # OI_LOCAL_LIGHT_MIN_DISTANCE
MARCH, MISS, BACKFACING = T.MARCH, T.MISS, T.BACKFACING

# the analytic cases on occlusion_ref's two-sphere scene (tests/test_local_light_cpu.py rehearses them): name -> position,
# radius, samples
ANALYTIC = {"below": ((0.0, 0.0, 0.65), 0.0, 1), "above": ((0.0, 0.0, 1.2), 0.0, 1), "sphere": ((0.0, 0.0, 1.2), 0.08, 64)}
ANALYTIC_BIAS = 1e-2

# the two local lights of the golden 24 x 24 views, placed relative to the view's eye so that they light the visible side (c:
# the unit vector from the object's centre to the eye in the box frame, s: a unit vector across it): one inside the unit
# sphere near the object, one sphere light outside it; the reference distances keep att of order 1 on the object, so the
# directional image's bar applies.  along / across: the position c * along + s * across in the box frame.
GOLDEN_LIGHTS = [dict(along=0.45, across=0.55, radius=0.0, reference_distance=0.35),
                 dict(along=0.9, across=-1.2, radius=0.15, reference_distance=1.2)]
GOLDEN_COLOURS = dict(ambient=(0.2, 0.25, 0.3), diffuse=(0.7, 0.6, 0.5), specular=(0.3, 0.2, 0.35), shininess=6.0)


def record(position, radius=0.0, ambient=(0.3, 0.3, 0.3), diffuse=(0.6, 0.6, 0.6), specular=(0.0, 0.0, 0.0), shininess=10.0,
           reference_distance=1.0, cone_axis=None, cone_inner=None, cone_outer=None):
    """The 20 floats of one light, as the header lays them out (angles in radians)."""
    if cone_axis is None:
        axis, co, ci = (0.0, 0.0, 0.0), -2.0, 2.0
    else:
        axis, co, ci = cone_axis, np.cos(cone_outer), np.cos(cone_inner)
    return [*position, radius, *ambient, reference_distance, *diffuse, co, *specular, shininess, *axis, ci]


def in_frame(lt, w2b):
    """-> q = w2b (position, 1) and the radius (NaN / negative -> 0) of the record lt."""
    lt, w2b = np.asarray(lt, dtype=np.float64), np.asarray(w2b, dtype=np.float64)
    r = lt[3]
    return w2b[:3, :3] @ lt[:3] + w2b[:3, 3], 0.0 if (np.isnan(r) or r < 0) else float(r)


def aimed(o, normals, pix, q, radius, S, seed, j0=0, Sc=None):
    """Samples j0 .. j0 + Sc - 1 of S from the origins o (n, 3) with the unit normals towards the sphere (q, radius), all in one
    frame.  -> dict of d (Sc, n, 3), t_light, ca (Sc, n), dc, cos_max (n,), axis (n, 3), inside (n,), facing (Sc, n)."""
    o, nrm = np.asarray(o, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    Sc = S if Sc is None else Sc
    w = np.asarray(q, dtype=np.float64) - o
    dc = np.linalg.norm(w, axis=-1)
    inside = dc <= radius
    safe = np.where(inside, 1.0, dc)
    axis = w / safe[:, None]
    axis[inside] = (0.0, 0.0, 1.0)                           # (not read: such a ray is never traced)
    sin_max = np.where(inside, 0.0, radius / safe)
    cos_max = np.sqrt((1.0 - sin_max) * (1.0 + sin_max))
    u1, u2 = R.sample_numbers(pix, seed, S)
    u1, u2 = u1[j0:j0 + Sc], u2[j0:j0 + Sc]
    m = u1[:, None] * (1.0 - cos_max)[None]
    ca, sa = 1.0 - m, np.sqrt(np.maximum(m * (2.0 - m), 0.0))
    ax = np.broadcast_to(axis, (Sc,) + axis.shape)
    d = np.where((sa == 0)[..., None], ax, R.directions(ax, sa, ca, u2))
    t_light = dc[None] * ca - np.sqrt(np.maximum(radius * radius - (dc[None] * sa) ** 2, 0.0))
    facing = (nrm[None] * d).sum(-1) > 0
    return dict(d=d, t_light=t_light, ca=ca, dc=dc, cos_max=cos_max, axis=axis, inside=inside, facing=facing)


def rays(points, grad, pix, lt, w2b, S, seed, bias=T.BIAS, j0=0, Sc=None):
    """oi_local_light_begin for one light record: -> dict of o, d (Sc, n, 3), far, t_light (Sc, n), status (Sc, n) with MARCH for
    an entered ray, and aimed()'s fields."""
    nrm = A.unit(np.asarray(grad, dtype=np.float64))
    o = np.asarray(points, dtype=np.float64) + bias * nrm
    q, radius = in_frame(lt, w2b)
    a = aimed(o, nrm, pix, q, radius, S, seed, j0, Sc)
    ob = np.broadcast_to(o, a["d"].shape)
    traced = a["facing"] & ~a["inside"][None]
    far = np.where(traced, np.minimum(a["t_light"], R.unit_sphere_exit(ob, a["d"])), 0.0)
    status = np.where(a["inside"][None], MISS, np.where(a["facing"], MARCH, BACKFACING)).astype(np.uint8)
    d = np.where(a["inside"][None, :, None], 0.0, a["d"])
    out = dict(a)
    out.update(o=ob, d=d, far=far, status=status, traced=traced, q=q, radius=radius)
    return out


def smoothstep(c, lo, hi):
    tt = np.clip((c - lo) / (hi - lo), 0.0, 1.0)
    return tt * tt * (3.0 - 2.0 * tt)


def factors(points, lt, w2b):
    """-> l (n, 3) the unit direction to the light, att, spot (n,) at box-frame points."""
    lt, w2b = np.asarray(lt, dtype=np.float64), np.asarray(w2b, dtype=np.float64)
    q, radius = in_frame(lt, w2b)
    u = q - np.asarray(points, dtype=np.float64)
    dist2 = (u * u).sum(-1)
    l = u / np.maximum(np.sqrt(dist2), 1e-6)[:, None]
    att = lt[7] ** 2 / np.maximum(dist2, max(radius, MIN_DISTANCE) ** 2)
    if lt[11] <= -1:
        spot = np.ones(len(u))
    else:
        a = w2b[:3, :3] @ (lt[16:19] / np.linalg.norm(lt[16:19]))
        spot = smoothstep(-(l @ a), lt[11], lt[19])
    return l, att, spot


def shade(eye, points, grad, rgb, w2b, lights, visibility=None, ao=None):
    """oi_surface_shade_local on hit rays, float64.  eye, points, grad, rgb (n, 3) in the box frame, lights (L, 20),
    visibility (L, n), ao (n,) -> image (L, 3, n)."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    eye, p, rgb = f(eye), f(points), f(rgb)
    nrm = A.unit(f(grad))
    v = eye - p
    v = v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-6)
    out = []
    for li, lt in enumerate(f(lights).reshape(-1, FLOATS)):
        l, att, spot = factors(p, lt, w2b)
        k = att * spot * (1.0 if visibility is None else f(visibility)[li])
        ndl = (nrm * l).sum(-1)
        r = -l + 2.0 * ndl[:, None] * nrm
        al = np.maximum((v * r).sum(-1), 0.0) * (ndl > 0)
        amb = lt[4:7][:, None] * (np.ones(len(p)) if ao is None else f(ao))[None]
        img = (amb + lt[8:11][:, None] * (np.maximum(ndl, 0.0) * k)[None]) * rgb.T + lt[12:15][:, None] * (al ** lt[15] * k)[None]
        out.append(img)
    return np.stack(out)


def other_element(o_world, d_owner, w2b_owner, w2b_other, t_light):
    """The scene's rule for e' != e: the world origin (n, 3) and the owner-frame directions (..., n, 3) moved into e''s frame,
    culled against its unit sphere and clipped to the light.  -> o, d, near, far, entered, c2."""
    We, Wb = np.asarray(w2b_owner, dtype=np.float64), np.asarray(w2b_other, dtype=np.float64)
    d_world = np.einsum("ba,...b->...a", We[:3, :3], np.asarray(d_owner, dtype=np.float64))
    d = np.einsum("ab,...b->...a", Wb[:3, :3], d_world)
    o = np.broadcast_to(SR.transform(Wb, np.asarray(o_world, dtype=np.float64)), d.shape)
    ent, near, far, c2 = SR.cull(o, d)
    ent = ent & (near < t_light)
    far = np.minimum(far, t_light)
    return o, d, np.where(ent, near, 0.0), np.where(ent, far, 0.0), ent, c2


def sphere_hit(o, d, far, c, r):
    """Does the segment o + t d, 0 <= t <= far (d unit) meet the sphere (c, r)?  Exact ray / sphere intersection; also the
    distance of the segment's closest point from c, for the tangency band."""
    oc = np.asarray(o, dtype=np.float64) - c
    b = (oc * d).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - r * r)
    t0 = -b - np.sqrt(np.maximum(disc, 0.0))
    t1 = -b + np.sqrt(np.maximum(disc, 0.0))
    hit = (disc > 0) & (t1 > 0) & (t0 < far)
    return hit, R.closest_approach(o, d, far, c)


def analytic_case(name, seed=R.SEED):
    """One of ANALYTIC on the 16 x 16 top patch of the two-sphere scene with exact intersection: -> dict of the rays, lit (S, n)
    (no sphere between the origin and the light), band (S, n) (within TANGENCY_BAND of tangency to either sphere), vis (n,),
    r_xy (n,), pix."""
    pos, radius, S = ANALYTIC[name]
    p, n = R.analytic_patch()
    pix = np.arange(len(p)) * 3 + 5
    r = rays(p, n * 2.5, pix, record(pos, radius), np.eye(4), S, seed, bias=ANALYTIC_BIAS)
    hit1, ca1 = sphere_hit(r["o"], r["d"], r["far"], R.C1, R.R1)
    hit0, ca0 = sphere_hit(r["o"], r["d"], r["far"], R.C0, R.R0)
    band = (np.abs(ca1 - R.R1) < R.TANGENCY_BAND) | (np.abs(ca0 - R.R0) < R.TANGENCY_BAND)
    lit = r["traced"] & ~hit1 & ~hit0
    r.update(lit=lit, band=band & r["traced"], vis=lit.mean(0), r_xy=np.linalg.norm(p[:, :2], axis=-1), pix=pix, points=p,
             grad=n * 2.5, S=S, light=record(pos, radius))
    return r


def golden_positions(pose_name, Rv=R.R_SOFT):
    """The WORLD positions of GOLDEN_LIGHTS for a golden view, from the oracle's own rays."""
    ro, _, _, _, w2b = T.view_rays(pose_name, Rv)
    c = ro[0] / np.linalg.norm(ro[0])
    s = np.cross(c, [0.0, 0.0, 1.0] if abs(c[2]) < 0.9 else [1.0, 0.0, 0.0])
    s /= np.linalg.norm(s)
    b2w = np.linalg.inv(w2b)
    return [b2w[:3, :3] @ (c * g["along"] + s * g["across"]) + b2w[:3, 3] for g in GOLDEN_LIGHTS]


def golden_records(pose_name, Rv=R.R_SOFT):
    return [record(tuple(p), g["radius"], reference_distance=g["reference_distance"], **GOLDEN_COLOURS)
            for p, g in zip(golden_positions(pose_name, Rv), GOLDEN_LIGHTS)]


def rehearse_golden(seed, pose_name, Rv=R.R_SOFT, S=R.SOFT_S):
    """The local shadow rays of one golden view on the oracle alone under GOLDEN_LIGHTS.  -> per light a dict of counts."""
    fld = T.Field(seed)
    ro, rd, near, far, w2b = T.view_rays(pose_name, Rv)
    t, status, _, _ = T.trace(fld.sdf, ro, rd, near, far)
    hit = status == T.HIT
    pix = np.nonzero(hit)[0]
    pts = ro[hit] + t[hit, None] * rd[hit]
    _, g, _ = fld.full(pts)
    out = {"n_hit": int(hit.sum())}
    for i, lt in enumerate(golden_records(pose_name, Rv)):
        r = rays(pts, g, pix, lt, w2b, S, R.SEED)
        m = r["traced"].reshape(-1)
        _, st, _, in_flight = R.trace_anyhit(fld.sdf, r["o"].reshape(-1, 3)[m], r["d"].reshape(-1, 3)[m], np.zeros(int(m.sum())),
                                             r["far"].reshape(-1)[m])
        out[f"light{i}"] = {"traced": int(m.sum()), "of": int(m.size), "limit": int((st == T.LIMIT).sum()),
                            "start_inside": int((st == T.START_INSIDE).sum()), "occluded": int((st == T.HIT).sum()),
                            "lit": int((st == T.MISS).sum()), "inside": int(r["inside"].sum()), "evals": int(sum(in_flight))}
    return out
