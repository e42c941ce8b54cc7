"""float64 numpy restatement of include/oi_scene_gloss.h, built from the existing restatements: the
reflected view vector, the lobe sampler, the lookup and the glossy shade of helpers.envgloss_ref, the per-element ray
construction of helpers.scene_light_ref (fed the lobe's directions through d_owner=) and the transform of helpers.scene_ref.
It restates the eye of every visible point, the lobe rays in every occluder element, the reflection plane and the shade
with given directions -- plus the lobe rays of the analytic two-sphere scene.  Nothing here touches the code under test."""
import numpy as np

from helpers import env_ref as EV
from helpers import envgloss_ref as Q
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T

AN_S = 64                     # samples per point of the analytic scene's lobe rays
AN_SHININESS = (1.0, 10.0)    # its two lobes
BLOCKED_FLOOR = 0.01          # share of sphere 0's facing lobe rays the other sphere must block
NDD_EDGE = 1e-5               # facing is compared only where |n . d| exceeds this


def point_eyes(rays_o, vis_index, offset, elem):
    """The eye of every visible point: rays_o (E, N, 3), vis_index (E, N), offset (E,), elem (n,) -> (n, 3): point g of element
    e = elem[g] at slot g - offset[e] was found by primary ray vis_index[e][slot], whose origin is the eye."""
    elem = np.asarray(elem)
    slot = np.arange(len(elem)) - np.asarray(offset)[elem]
    return np.asarray(rays_o, dtype=np.float64)[elem, np.asarray(vis_index)[elem, slot]]


def owner_lobe_directions(points, grad, eyes, offset, elem, pixel, S, j0, Sc, s, seed):
    """Samples j0 .. j0 + Sc - 1 of S of every visible point's lobe, in its owner's frame: -> (1, Sc, n, 3), the normals (n, 3)
    and the reflected view vectors (n, 3)."""
    elem = np.asarray(elem)
    slot = np.arange(len(elem)) - np.asarray(offset)[elem]
    n, _, r = Q.reflect(np.asarray(grad, dtype=np.float64)[elem, slot], np.asarray(points, dtype=np.float64)[elem, slot], eyes)
    return Q.lobe_directions(r, np.asarray(pixel), S, s, seed)[j0:j0 + Sc][None], n, r


def lobe_rays(points, grad, eyes, offset, elem, pixel, position, normal_world, w2b, bias, S, j0, Sc, s, seed, d_owner=None):
    """oi_scene_lobe_begin: scene_light_ref.rays' dict for the lobe's directions (d_owner: the kernel's own, to restate the rest
    of the construction on them), the ambient form without a distance limit."""
    if d_owner is None:
        d_owner, _, _ = owner_lobe_directions(points, grad, eyes, offset, elem, pixel, S, j0, Sc, s, seed)
    return SL.rays(points, grad, offset, elem, pixel, position, normal_world, w2b, bias, S, j0, Sc, seed, distance=np.inf,
                   d_owner=d_owner)


def reflection(rays_o, points, grad, owner, owner_ray, vis_slot, w2b):
    """oi_scene_reflect: -> (M, 3) world frame, zeros off the mask."""
    owner, owner_ray = np.asarray(owner), np.asarray(owner_ray)
    out = np.zeros((len(owner), 3))
    on = np.nonzero(owner >= 0)[0]
    e, ray = owner[on], owner_ray[on]
    k = np.asarray(vis_slot)[e, ray]
    _, _, r = Q.reflect(np.asarray(grad, dtype=np.float64)[e, k], np.asarray(points, dtype=np.float64)[e, k],
                        np.asarray(rays_o, dtype=np.float64)[e, ray])
    out[on] = np.einsum("nba,nb->na", np.asarray(w2b, dtype=np.float64)[e][:, :3, :3], r)       # w2b_e[:3,:3]^T r
    return out


def shade_dirs(transfer_map, envs, mask, albedo, dirs, spec_vis, maps, map_index, rot, k_s, bg=None):
    """oi_env_shade_glossy_dirs: envgloss_ref.shade_glossy with the world-frame direction of every pixel given, dirs (N, 3).
    -> shading, image, specular (F, 3, N), the diffuse magnitude, the lookups (F, 3, N) and the lookup directions (F, N, 3)."""
    sh, img, mag = EV.shade(transfer_map, envs, mask, albedo, bg)
    F, N = len(envs), len(mask)
    m = np.asarray(mask, dtype=bool)
    d = np.einsum("nk,fkj->fnj", np.asarray(dirs, dtype=np.float64), np.asarray(rot, dtype=np.float64))   # R_f^T r_w
    look = np.zeros((F, 3, N))
    for f in range(F):
        if m.any():
            look[f][:, m] = Q.lookup(np.asarray(maps)[map_index[f]], d[f][m]).T
    vis = np.ones(N) if spec_vis is None else np.asarray(spec_vis, dtype=np.float64)
    spec = np.asarray(k_s, dtype=np.float64)[None, :, None] * vis[None, None, :] * look
    img = np.where(m[None, None, :], img + spec, img)
    return sh, img, spec, mag, look, d


def analytic_eyes(sc, pts):
    """The eye of the analytic scene's points in each owner's frame: the camera centre (every primary ray starts there)."""
    o, _ = SR.scene_rays(sc["c2w"], sc["K_inv"], sc["S"])
    eye_w = np.asarray(o, dtype=np.float64).reshape(-1, 3)[0]
    w2b = pts["w2b"][pts["e"]]
    return np.einsum("nab,b->na", w2b[:, :3, :3], eye_w) + w2b[:, :3, 3], eye_w


def analytic_lobe(sc, pts, S, s, seed, bias=T.BIAS):
    """The lobe rays of the analytic scene's points in float64, drawn in the owner's frame about the reflected view vector and
    taken to the world: scene_light_ref.analytic_secondary's dict."""
    e, w2b = pts["e"], pts["w2b"]
    eyes, _ = analytic_eyes(sc, pts)
    p_obj = np.einsum("nab,nb->na", w2b[e][:, :3, :3], pts["p"]) + w2b[e][:, :3, 3]
    _, _, r = Q.reflect(pts["n_obj"], p_obj, eyes)
    d_obj = Q.lobe_directions(r, pts["q"], S, s, seed)
    d_world = np.einsum("nba,snb->sna", w2b[e][:, :3, :3], d_obj)
    ndd = (pts["nw"][None] * d_world).sum(-1)
    facing = ndd > 0
    o = np.broadcast_to(pts["p"] + bias * pts["nw"], d_world.shape)
    blocked, band = SL.sphere_blocks(o, d_world)
    return dict(d_world=d_world, facing=facing, ndd=ndd, free=facing & ~blocked.any(0), blocked_by=blocked,
                in_band=band.any(0) & facing)
