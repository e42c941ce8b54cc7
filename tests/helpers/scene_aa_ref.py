"""CPU restatement of the anti-aliasing stage of a scene of many instances (include/oi_scene_aa.h), which
touches no code under test:

    classify       the four criteria in numpy fp32: mask and instance on the owner map, plane and normal by aa_ref's
                   arithmetic (every product and sum rounded on its own, associated as include/oi_aa.h states them) on pairs
                   one instance owns, so the flagged set is the kernel's bit for bit
    dense          one instance's owner map as the status / hit_slot arrays aa_ref.classify takes
    virtual_size   the side Q of the virtual scene image of the sub-samples
    sub_rays       per instance the sub-pixel rays in float64, the primary's window rule and scene_ref.cull
    analytic_sub   the closed form of the analytic two-sphere scene per sub-sample ray, with scene_ref's exclusions"""
import math

import numpy as np

from helpers import aa_ref as AR
from helpers import scene_ref as SR

f32 = np.float32


def owned_rows(owner, owner_ray, vis_slot, n_pad):
    """-> (owned (M,) bool, e (M,), row (M,): the row e * n_pad + slot of the pixel's visible hit; 0 where not owned).
    include/oi_scene_aa.h's owned(p): anything out of range reads as not owned."""
    owner, owner_ray = np.asarray(owner, np.int64), np.asarray(owner_ray, np.int64)
    vis_slot = np.asarray(vis_slot, np.int64)
    E, N = vis_slot.shape
    ok = (owner >= 0) & (owner < E) & (owner_ray >= 0) & (owner_ray < N)
    e, r = np.where(ok, owner, 0), np.where(ok, owner_ray, 0)
    k = vis_slot[e, r]
    ok &= (k >= 0) & (k < n_pad)
    return ok, np.where(ok, e, 0), np.where(ok, e * n_pad + k, 0)


def dense(owner, owner_ray, vis_slot, n_pad):
    """The scene's owner map as ONE traced view: status (HIT where owned) and hit_slot (the row in the flattened (E * n_pad, 3)
    arrays), what aa_ref.classify takes."""
    ok, _, row = owned_rows(owner, owner_ray, vis_slot, n_pad)
    return np.where(ok, AR.HIT, 0).astype(np.uint8), np.where(ok, row, -1).astype(np.int32)


def classify(owner, owner_ray, vis_slot, points, grad, S, plane=AR.DEFAULT_PLANE, cos=AR.DEFAULT_COS, parts=False):
    """owner, owner_ray (S * S,), vis_slot (E, N), points and grad (E, n_pad, 3).  -> flagged (S * S,) bool.  parts: -> the
    (mask, instance, plane, normal) criteria separately."""
    n_pad = 0 if points is None else np.asarray(points).shape[1]
    ok, e, row = owned_rows(owner, owner_ray, vis_slot, n_pad)
    hit, e = ok.reshape(S, S), e.reshape(S, S)
    pts, g = np.zeros((S, S, 3), f32), np.zeros((S, S, 3), f32)
    if n_pad:
        pts = np.where(ok[:, None], np.asarray(points, f32).reshape(-1, 3)[row], 0).astype(f32).reshape(S, S, 3)
        g = np.where(ok[:, None], np.asarray(grad, f32).reshape(-1, 3)[row], 0).astype(f32).reshape(S, S, 3)
    gg = AR._dot(g, g)
    s2, c2 = f32(plane) * f32(plane), f32(cos) * f32(cos)
    out = [np.zeros((S, S), bool) for _ in range(4)]

    def window(a, dy, dx):
        ys, xs = slice(max(0, -dy), S - max(0, dy)), slice(max(0, -dx), S - max(0, dx))
        yq, xq = slice(max(0, dy), S - max(0, -dy)), slice(max(0, dx), S - max(0, -dx))
        return a[ys, xs], a[yq, xq], (ys, xs)

    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy == 0 and dx == 0:
                    continue
                hp, hq, at = window(hit, dy, dx)
                ep, eq, _ = window(e, dy, dx)
                xp, xq, _ = window(pts, dy, dx)
                gp, gq, _ = window(g, dy, dx)
                gpp, gqq, _ = window(gg, dy, dx)
                both = hp & hq
                same = both & (ep == eq)
                u = xq - xp
                uu = AR._dot(u, u)
                dp, dq = AR._dot(gp, u), AR._dot(gq, u)
                off = (dp * dp > (s2 * gpp) * uu) | (dq * dq > (s2 * gqq) * uu)
                d = AR._dot(gp, gq)
                turned = (d <= 0) | (d * d < (c2 * gpp) * gqq)
                out[0][at] |= hp != hq
                out[1][at] |= both & (ep != eq)
                out[2][at] |= same & off
                out[3][at] |= same & turned
    out = [o.reshape(-1) for o in out]
    return tuple(out) if parts else out[0] | out[1] | out[2] | out[3]


def virtual_size(n_sub):
    """The smallest Q with Q * Q >= n_sub, in integers."""
    Q = math.isqrt(n_sub)
    return Q if Q * Q == n_sub else Q + 1


def sub_rays(c2b, kinv, S, W, origins, pixels, offsets):
    """Per instance the sub-pixel rays of the scene pixels `pixels` (Y * S + X) at offsets (Sa, 2), float64: ray (j - 1) * n + k
    is sample j of pixels[k].  c2b (E, 4, 4), origins (E, 2).  -> o (E, n_sub, 3), d (E, n_sub, 3), covered (E, n_sub) (the
    window of e holds the PIXEL), entered = covered and scene_ref.cull, near, far (0 where not entered)."""
    c2b, pixels = np.asarray(c2b, np.float64).reshape(-1, 4, 4), np.asarray(pixels, np.int64)
    Sa = len(offsets)
    X, Y = np.tile(pixels % S, Sa - 1), np.tile(pixels // S, Sa - 1)
    o, d, cov = [], [], []
    for e, m in enumerate(c2b):
        oe, de, _, _ = AR.sub_rays(m, kinv, (0.0, 0.0), S, pixels, offsets)
        o.append(oe), d.append(de)
        i, j = X - origins[e][0], Y - origins[e][1]
        cov.append((i >= 0) & (i < W) & (j >= 0) & (j < W))
    o, d, cov = np.array(o), np.array(d), np.array(cov)
    ent, near, far, _ = SR.cull(o, d)
    ent &= cov
    return o, d, cov, ent, np.where(ent, near, 0.0), np.where(ent, far, 0.0)


def analytic_sub(sc, pixels, offsets):
    """The closed form of scene_ref's analytic two-sphere scene for the sub-sample rays of `pixels`: -> owner (n_sub,) (-1: none;
    a sphere counts only where its window holds the pixel) and the exclusion mask with scene_ref's own exclusions (the closest
    approach within AN_SILHOUETTE of a silhouette, two depths within AN_DEPTH_GAP)."""
    S, W = sc["S"], sc["W"]
    o, d, _, _ = AR.sub_rays(sc["c2w"], sc["K_inv"], (0.0, 0.0), S, pixels, offsets)
    Sa = len(offsets)
    X, Y = np.tile(np.asarray(pixels) % S, Sa - 1), np.tile(np.asarray(pixels) // S, Sa - 1)
    ts, near_rim = [], np.zeros(len(d), bool)
    for e, c in enumerate(SR.AN_CENTRES):
        oc = o - c
        b = (d * oc).sum(-1)
        perp2 = (oc * oc).sum(-1) - b * b
        disc = SR.RADIUS ** 2 - perp2
        i, j = X - sc["origins"][e][0], Y - sc["origins"][e][1]
        cov = (i >= 0) & (i < W) & (j >= 0) & (j < W)
        ts.append(np.where((disc > 0) & cov, -b - np.sqrt(np.maximum(disc, 0.0)), np.inf))
        near_rim |= cov & (np.abs(np.sqrt(perp2) - SR.RADIUS) < SR.AN_SILHOUETTE)
    ts = np.array(ts)
    owner = np.where(np.isfinite(ts).any(0), ts.argmin(0), -1)
    both = np.isfinite(ts).all(0)
    gap = np.abs(np.where(both, ts[0], 0.0) - np.where(both, ts[1], 0.0))
    return owner, near_rim | (both & (gap < SR.AN_DEPTH_GAP))
