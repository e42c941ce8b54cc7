"""float64 numpy restatement of include/oi_scene_bounce.h, built from the existing restatements: the
pixel lists and the analytic secondary rays of helpers.scene_light_ref, the basis, A_HAT and the world rotation of
helpers.env_ref, the term roundings and the bars of helpers.bounce_ref.  It covers the winner of a sample, the per-element
selection, the accumulation of the bounce transfer over chunks of samples -- plus the exact secondary hits of the analytic
two-sphere scene (helpers.scene_ref.analytic_scene).  Nothing here touches the code under test."""
import numpy as np

from helpers import bounce_ref as B
from helpers import env_ref as EV
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T

MISS, HIT = T.MISS, T.HIT
EPS = B.EPS
# the analytic scene's albedo per sphere: a white one beside a red one
AN_ALBEDO = np.array([[1.0, 1.0, 1.0], [1.0, 0.1, 0.1]])
AN_SEED = SL.SEED            # 7: tests/test_scene_bounce_cpu.py rehearses the exclusion cap at this seed
AN_SAMPLES = (16, 64)
NDD_EDGE = 1e-3              # |n . d| at a secondary hit below which float32 may decide the face either way
EXCLUDED_CAP = 0.01


def winners(status, t):
    """oi_scene_bounce_nearest: status, t (E, ...) -> winner (...) int: -1 when any element's status is neither MISS nor HIT;
    otherwise the element with a HIT and the smallest t, the lowest index on equal t (a later element replaces the winner only
    when its t is strictly smaller); -1 without a HIT."""
    status, t = np.asarray(status), np.asarray(t, dtype=np.float64)
    best = np.full(status.shape[1:], -1, dtype=np.int64)
    best_t = np.full(status.shape[1:], np.inf)
    dead = np.zeros(status.shape[1:], dtype=bool)
    for e in range(status.shape[0]):
        hit = status[e] == HIT
        dead |= ~hit & (status[e] != MISS)
        better = hit & ((best < 0) | (t[e] < best_t))
        best = np.where(better, e, best)
        best_t = np.where(better, t[e], best_t)
    return np.where(dead, -1, best)


def selection(winner, E):
    """oi_scene_bounce_visible: winner (Nr,) -> per element the sorted rays it wins (the kernel's order is not fixed)."""
    w = np.asarray(winner)
    return [np.nonzero(w == e)[0] for e in range(E)]


def slots_consistent(winner, sel_index, sel_slot, counts):
    """Is (sel_index, sel_slot, counts) a consistent dense list per element for `winner`?  sel_index, sel_slot (E, Nr).
    -> None, or a text that names the first defect."""
    w = np.asarray(winner)
    for e, rays in enumerate(selection(w, len(sel_slot))):
        if counts[e] != len(rays):
            return f"element {e}: count {counts[e]}, {len(rays)} rays won"
        if sorted(np.asarray(sel_index[e][:counts[e]]).tolist()) != rays.tolist():
            return f"element {e}: the listed rays are not the rays won"
        slot = np.asarray(sel_slot[e])
        if (slot[w != e] != -1).any():
            return f"element {e}: a slot for a ray it does not win"
        if not np.array_equal(np.asarray(sel_index[e])[slot[rays]], rays):
            return f"element {e}: sel_index[sel_slot[q]] != q"
    return None


def resolve(chunks, owner, owner_ray, vis_slot, offset, w2b, S):
    """oi_scene_bounce_resolve over the chunks, in order.  A chunk: dict(winner (Sc, n_vis), sel_slot (E, Sc, n_vis), rays_d
    (E, Sc, n_vis, 3), grad2, rgb2 (E, n_pad2, 3) or None).  -> the bounce transfer (3, 9, M); the mean over a pixel's samples of
    [front-face winner] |rho| A_Y_MAX (3, 9, M), which the bar scales with; per chunk n . d (Sc, pixels on the mask) (0 without
    a winner) and the front-face winners (Sc, pixels on the mask)."""
    M = len(owner)
    on, g = SL.pixel_points(owner, owner_ray, vis_slot, offset)
    out, mag = np.zeros((3, EV.N_COEFFS, M)), np.zeros((3, EV.N_COEFFS, M))
    rot = np.asarray(w2b, dtype=np.float64)[:, :3, :3]
    ndds, fronts = [], []
    for ch in chunks:
        w = np.asarray(ch["winner"])[:, g]                                     # (Sc, pixels)
        Sc = w.shape[0]
        n2 = 0 if ch.get("grad2") is None else ch["grad2"].shape[1]
        if n2 == 0:
            ndds.append(np.zeros(w.shape)), fronts.append(np.zeros(w.shape, dtype=bool))
            continue
        E = len(rot)
        jj = np.broadcast_to(np.arange(Sc)[:, None], w.shape)
        gg = np.broadcast_to(g[None], w.shape)
        has = (w >= 0) & (w < E)
        ww = np.where(has, w, 0)
        k = np.asarray(ch["sel_slot"])[ww, jj, gg].astype(np.int64)
        ok = has & (k >= 0) & (k < n2)
        kk = np.where(ok, k, 0)
        grad = np.asarray(ch["grad2"], dtype=np.float64)[ww, kk]
        n = grad / np.maximum(np.linalg.norm(grad, axis=-1, keepdims=True), 1e-6)
        d = np.asarray(ch["rays_d"], dtype=np.float64)[ww, jj, gg]
        nd = np.where(ok, (n * d).sum(-1), 0.0)
        front = ok & (nd < 0)
        nw = np.einsum("spba,spb->spa", rot[ww], n)                             # w2b_w[:3,:3]^T n
        t = EV.closed_form(nw)
        rho = np.asarray(ch["rgb2"], dtype=np.float64)[ww, kk] * front[..., None]
        out[:, :, on] += np.einsum("spk,spc->kcp", rho, t)
        mag[:, :, on] += np.einsum("spk,c->kcp", np.abs(rho), B.A_Y_MAX)
        ndds.append(nd), fronts.append(front)
    return out / S, mag / S, ndds, fronts


resolve_bar = B.resolve_bar      # (K_band + S + 2) eps mag per output, K = 1 / 14 / 40: section 4.22's derivation, the same term


# ---------------------------------------------------------------------------------------------------------------------
# the analytic two-sphere scene: exact secondary hits
# ---------------------------------------------------------------------------------------------------------------------
def sphere_hits(o, d):
    """Nearest intersection of world rays (o, d) (unit d, any leading shape) with each sphere of the analytic scene: -> t
    (2, ...) (inf without one in front of the origin)."""
    ts = []
    for c in SR.AN_CENTRES:
        oc = o - c
        b = -(oc * d).sum(-1)
        disc = b * b - ((oc * oc).sum(-1) - SR.RADIUS ** 2)
        t = b - np.sqrt(np.maximum(disc, 0.0))
        ts.append(np.where((disc > 0) & (t > 0), t, np.inf))
    return np.stack(ts)


def analytic_bounce(sc, pts, S, seed, albedo=AN_ALBEDO, bias=T.BIAS):
    """The analytic scene's bounce in float64 on exact intersections: scene_light_ref.analytic_secondary's world rays, the
    nearest of the two spheres, the normal (y - c) / 0.5, a constant albedo per sphere.  -> dict: winner (S, n) (-1: free or
    facing away), y (S, n, 3), normal (S, n, 3), ndd (S, n) at the secondary hit, excluded (S, n): facing rays in the band
    |closest approach - 0.5| < AN_SHADOW_EDGE or with |n . d| < NDD_EDGE at the hit, facing (S, n), T1 (3, 9, n) per point."""
    a = SL.analytic_secondary(sc, pts, S, seed, bias=bias)
    d = a["d_world"]
    o = np.broadcast_to(pts["p"] + bias * pts["nw"], d.shape)
    t = sphere_hits(o, d)
    hit = np.isfinite(t).any(0) & a["facing"]
    w = np.where(hit, t.argmin(0), -1)
    tt = np.where(hit, t.min(0), 0.0)
    y = o + tt[..., None] * d
    nrm = (y - SR.AN_CENTRES[np.maximum(w, 0)]) / SR.RADIUS
    ndd = np.where(hit, (nrm * d).sum(-1), 0.0)
    excluded = a["in_band"] | (hit & (np.abs(ndd) < NDD_EDGE))
    front = hit & (ndd < 0)
    rho = np.asarray(albedo, dtype=np.float64)[np.maximum(w, 0)] * front[..., None]
    T1 = np.einsum("snk,snc->kcn", rho, EV.closed_form(nrm)) / S
    return dict(winner=w, y=y, normal=nrm, ndd=ndd, excluded=excluded, facing=a["facing"], front=front, T1=T1, d_world=d, o_world=o)
