"""float64 numpy restatement of include/oi_scene_light.h, built from the existing restatements: the
sample numbers and directions of helpers.occlusion_ref, the transform and the cull of helpers.scene_ref, the SH basis of
helpers.env_ref.  It covers the construction of the sampled rays per occluder element, the combination across elements, and
the accumulation of counts and transfer vectors over chunks of samples -- plus the closed forms of the analytic two-sphere
scene's secondary rays.  Nothing here touches the code under test."""
import numpy as np

from helpers import env_ref as EV
from helpers import occlusion_ref as R
from helpers import scene_ref as SR
from helpers import trace_ref as T

MISS, HIT, BACKFACING, MARCH = T.MISS, T.HIT, T.BACKFACING, T.MARCH
SEED = 7
# the analytic scene's settings (tests/test_scene_light_cpu.py rehearses them on float64 alone)
AN_AO_S, AN_TRANSFER_S, AN_SOFT_S, AN_SOFT_RADIUS = 16, 64, 4, 0.1
BLOCKED_FLOOR = 0.05         # share of sphere 0's ambient rays the other sphere must block, so the scene pins occlusion


def unit(g):
    """g / max(|g|, 1e-6): the kernels' normal."""
    g = np.asarray(g, dtype=np.float64)
    return g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-6)


def point_pixels(vis_index, window, W, S, offset, n_vis):
    """oi_scene_point_pixels: vis_index (E, N), window (E, 2), offset (E,), n_vis per element -> (sum n_vis,) scene pixels."""
    out = np.zeros(int(sum(n_vis)), dtype=np.int64)
    for e, n in enumerate(n_vis):
        r = np.asarray(vis_index[e][:n], dtype=np.int64)
        j, i = np.divmod(r, W)
        out[offset[e] + np.arange(n)] = (window[e][1] + j) * S + window[e][0] + i
    return out


def owner_directions(normals, pixel, seed, S, j0, Sc, axes=None, radius=None):
    """The directions of samples j0 .. j0 + Sc - 1 of S in the owner's frame.  normals (n, 3) unit, pixel (n,).  axes None:
    the cosine hemisphere about the normals -> (1, Sc, n, 3).  axes (L, n, 3) (each light's unit direction in the frame of
    each point's owner) and radius (L,): the caps -> (L, Sc, n, 3)."""
    u1, u2 = R.sample_numbers(pixel, seed, S)
    u1, u2 = u1[j0:j0 + Sc], u2[j0:j0 + Sc]
    if axes is None:
        return R.hemisphere_directions(np.asarray(normals, dtype=np.float64), u1, u2)[None]
    out = []
    for l, rad in enumerate(radius):
        cos_a = 1.0 - u1 * (1.0 - np.cos(R.clamp_radius(rad)))
        sin_a = np.sqrt(np.maximum(0.0, 1.0 - cos_a * cos_a))
        a = np.broadcast_to(np.asarray(axes[l], dtype=np.float64), u2.shape + (3,))
        out.append(R.directions(a, np.broadcast_to(sin_a[:, None], u2.shape), np.broadcast_to(cos_a[:, None], u2.shape), u2))
    return np.stack(out)


def light_axes(light_dirs, w2b, elem):
    """(L, n, 3): each world light direction in the frame of each point's owner."""
    return np.stack([np.stack([T.light_object_dir(d, w2b[e]) for e in range(len(w2b))])[elem] for d in light_dirs])


def rays(points, grad, offset, elem, pixel, position, normal_world, w2b, bias, S, j0, Sc, seed, light_dirs=None, radius=None,
         distance=None, d_owner=None):
    """oi_scene_occlusion_begin.  points, grad (E, n_pad, 3); elem, pixel (n,); position, normal_world (n, 3); w2b (E, 4, 4).
    light_dirs (L, 3) world + radius (L,), or distance (the ambient form, L = 1).  d_owner: directions to use instead of
    drawing them (the kernel's own, to restate the rest of the construction on its inputs).
    -> dict: d_owner (L, Sc, n, 3); per occluder element o, d (E, L, Sc, n, 3), near, far, c2 (E, L, Sc, n), status (E, L, Sc,
    n) with MARCH for an entered ray, traced (L, Sc, n)."""
    w2b = np.asarray(w2b, dtype=np.float64)
    E, n = len(w2b), len(elem)
    elem = np.asarray(elem)
    slot = np.arange(n) - np.asarray(offset)[elem]
    p = np.asarray(points, dtype=np.float64)[elem, slot]
    nrm = unit(np.asarray(grad, dtype=np.float64)[elem, slot])
    ambient = light_dirs is None
    if d_owner is None:
        d_owner = owner_directions(nrm, pixel, seed, S, j0, Sc, None if ambient else light_axes(light_dirs, w2b, elem), radius)
    d_owner = np.asarray(d_owner, dtype=np.float64)
    L = d_owner.shape[0]
    traced = (nrm[None, None] * d_owner).sum(-1) > 0
    rot = w2b[:, :3, :3]
    d_world = np.einsum("nba,lsnb->lsna", rot[elem], d_owner)                 # w2b_e[:3,:3]^T d
    o_world = np.asarray(position, dtype=np.float64) + bias * np.asarray(normal_world, dtype=np.float64)
    shape = (E, L, Sc, n)
    o, d = np.zeros(shape + (3,)), np.zeros(shape + (3,))
    near, far, c2 = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    status = np.full(shape, BACKFACING, dtype=np.uint8)
    own_o = p + bias * nrm
    for e in range(E):
        oe = np.broadcast_to(SR.transform(w2b[e], o_world), (L, Sc, n, 3))
        de = np.einsum("ab,lsnb->lsna", rot[e], d_world)
        ent, ne, fa, cc = SR.cull(oe, de)
        if ambient:
            ent = ent & (ne < distance)
            fa = np.minimum(fa, distance)
        mine = np.broadcast_to(elem == e, (L, Sc, n))
        own_far = R.unit_sphere_exit(np.broadcast_to(own_o, (L, Sc, n, 3)), d_owner)
        if ambient:
            own_far = np.minimum(own_far, distance)
        o[e] = np.where(mine[..., None], own_o, oe)
        d[e] = np.where(mine[..., None], d_owner, de)
        ent = np.where(mine, True, ent)
        near[e] = np.where(mine, 0.0, np.where(ent, ne, 0.0))
        far[e] = np.where(mine, own_far, np.where(ent, fa, 0.0))
        c2[e] = np.where(mine, 0.0, cc)
        status[e] = np.where(traced, np.where(ent, MARCH, MISS), BACKFACING)
    keep = traced[None, ..., None]
    o = np.where(keep, o, np.broadcast_to(own_o, o.shape))                    # a ray facing away keeps the owner's ray, not entered
    d = np.where(keep, d, np.broadcast_to(d_owner[None], d.shape))
    near, far = np.where(traced[None], near, 0.0), np.where(traced[None], far, 0.0)
    return dict(d_owner=d_owner, o=o, d=d, near=near, far=far, c2=c2, status=status, traced=traced)


def escaped(status):
    """status (E, ...) -> (...): the ray ended MISS in every element."""
    return (np.asarray(status) == MISS).all(0)


def pixel_points(owner, owner_ray, vis_slot, offset):
    """The scene pixels on the mask and the visible point of each."""
    on = np.nonzero(np.asarray(owner) >= 0)[0]
    return on, np.asarray(offset)[owner[on]] + np.asarray(vis_slot)[owner[on], owner_ray[on]]


def counts(chunks, owner, owner_ray, vis_slot, offset, S):
    """oi_scene_occlusion_resolve over the chunks' finished states, each (E, L, Sc, n_vis), in order.  -> count (L, M) int,
    out (L, M): count / S in float32 on the mask, 1 off it."""
    L, M = chunks[0].shape[1], len(owner)
    on, g = pixel_points(owner, owner_ray, vis_slot, offset)
    count = np.zeros((L, M), dtype=np.int64)
    for st in chunks:
        count[:, on] += escaped(st)[:, :, g].sum(1)
    out = np.ones((L, M))
    out[:, on] = (count[:, on].astype(np.float32) / np.float32(S)).astype(np.float64)
    return count, out


def transfer(chunks, owner, owner_ray, vis_slot, offset, w2b, S):
    """oi_scene_transfer_resolve over the chunks (status (E, 1, Sc, n_vis), the owner's-frame directions (1, Sc, n_vis, 3)),
    in order.  -> (9, M): the sum over the escaped samples of basis(normalize(w2b_owner[:3,:3]^T d)), divided by S; and the
    sum of |basis| over those samples (9, M), which the rounding bar scales with."""
    M = len(owner)
    on, g = pixel_points(owner, owner_ray, vis_slot, offset)
    acc, mag = np.zeros((EV.N_COEFFS, M)), np.zeros((EV.N_COEFFS, M))
    rot = np.asarray(w2b, dtype=np.float64)[:, :3, :3]
    for st, d in chunks:
        esc = escaped(st)[0][:, g]                                            # (Sc, pixels)
        v = np.einsum("nba,snb->sna", rot[owner[on]], np.asarray(d, dtype=np.float64)[0][:, g])
        y = EV.basis(v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-6))
        acc[:, on] += (esc[..., None] * y).sum(0).T
        mag[:, on] += (esc[..., None] * np.abs(y)).sum(0).T
    return acc / S, mag


# ---------------------------------------------------------------------------------------------------------------------
# the analytic two-sphere scene (helpers.scene_ref.analytic_scene): closed forms of its secondary rays
# ---------------------------------------------------------------------------------------------------------------------
def segment_closest(o, d, far, c):
    """Distance from c to the closest point of each segment o + t d, 0 <= t <= far (far may be inf)."""
    dd = (d * d).sum(-1)
    tc = np.clip(((c - o) * d).sum(-1) / dd, 0.0, far)
    return np.linalg.norm(o + tc[..., None] * d - c, axis=-1)


def sphere_blocks(o_world, d_world, distance=np.inf):
    """Per sphere of the analytic scene: does it block the world-frame rays (o, d), within `distance`?  -> blocked (2, ...),
    in_band (2, ...): |closest approach - radius| < AN_SHADOW_EDGE, where float32 may decide either way."""
    ca = np.stack([segment_closest(o_world, d_world, distance, c) for c in SR.AN_CENTRES])
    return ca < SR.RADIUS, np.abs(ca - SR.RADIUS) < SR.AN_SHADOW_EDGE


def analytic_points(sc, cf):
    """The visible points of the analytic scene on the closed form: per non-excluded owned pixel its scene pixel q, owner e,
    world point, world normal and object-frame normal."""
    S = sc["S"]
    o, d = SR.scene_rays(sc["c2w"], sc["K_inv"], S)
    d = d.reshape(-1, 3)
    q = np.nonzero((cf["owner"] >= 0) & ~cf["excluded"])[0]
    e = cf["owner"][q]
    p = o + cf["depth"][q, None] * d[q]
    nw = (p - SR.AN_CENTRES[e]) / SR.RADIUS
    w2b = np.stack([SR.rigid_inverse(m) for m in sc["b2w"]])
    n_obj = np.einsum("nab,nb->na", w2b[e][:, :3, :3], nw)
    return dict(q=q, e=e, p=p, nw=nw, n_obj=n_obj, w2b=w2b)


def analytic_secondary(sc, pts, S, seed, light=None, radius=None, distance=np.inf, bias=T.BIAS):
    """The sampled rays of the analytic scene's points in float64: directions drawn in the owner's frame (as the kernel
    draws them) and taken to the world.  -> d_world (S, n, 3), facing (S, n), free (S, n): facing and blocked by neither
    sphere, in_band (S, n): some sphere decides within the band."""
    e, w2b = pts["e"], pts["w2b"]
    axes = None if light is None else light_axes([light], w2b, e)
    d_obj = owner_directions(pts["n_obj"], pts["q"], seed, S, 0, S, axes, None if light is None else [radius])[0]
    d_world = np.einsum("nba,snb->sna", w2b[e][:, :3, :3], d_obj)
    facing = (pts["nw"][None] * d_world).sum(-1) > 0
    o = np.broadcast_to(pts["p"] + bias * pts["nw"], d_world.shape)
    blocked, band = sphere_blocks(o, d_world, distance)
    return dict(d_world=d_world, facing=facing, ndd=(pts["nw"][None] * d_world).sum(-1), free=facing & ~blocked.any(0),
                blocked_by=blocked, in_band=band.any(0) & facing)
