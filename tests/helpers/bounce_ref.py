"""fp64 numpy restatement of include/oi_envbounce.h: the bounce transfer of a finished closest-hit trace
(oi_bounce_resolve), the shading with it (oi_env_shade_bounce), the bars the GPU tests derive from the kernels' operation
sequences -- plus the bounce transfer of the analytic two-sphere scene of tests/helpers/env_ref.py: its S-sample estimator
with analytic ray / sphere intersections and normals, and its quadrature.  Builds on env_ref's basis, world_directions and
A_HAT; nothing here touches the code under test."""
import numpy as np

from helpers import env_ref as E
from helpers import occlusion_ref as R
from helpers import trace_ref as T

EPS = 2.0 ** -24
# the largest magnitude of each basis function over the sphere
Y_MAX = np.array([0.5 / np.sqrt(np.pi)] + [np.sqrt(3.0 / (4.0 * np.pi))] * 3 +
                 [0.5 * np.sqrt(15.0 / (4.0 * np.pi))] * 2 + [2.0 * np.sqrt(5.0 / (16.0 * np.pi))] +
                 [0.5 * np.sqrt(15.0 / (4.0 * np.pi)), np.sqrt(15.0 / (16.0 * np.pi))])
A_Y_MAX = E.A_HAT[E.BAND] * Y_MAX                  # the largest magnitude of one sample's A_band y_c
# Roundings (of at most 2^-24 relative each) behind ONE term A_band(c) y_c(n_w) of oi_bounce_resolve, in units of A_Y_MAX[c]:
#   normalise   3 products, 2 additions, a square root, a division                                       7
#   rotate      3 products, 2 additions, on components of magnitude <= 1                                  5
#               -> every component of n_w is within 12 roundings of its value
#   basis       band 0: the constant itself (1).  Band 1: the 12 pass through (|dy/dn| = k1 = Y_MAX), the product by k1 and
#               the product by 2/3 (14).  Band 2: a quadratic form, its gradient over its maximum is at most 3 (y6: 6 |z| / 2;
#               2 sqrt(2) for the others), so 3 * 12, and at most 4 operations of its own; 1/4 is exact (40)
TERM_ROUNDINGS = np.array([1.0, 14.0, 40.0])[E.BAND]


def resolve(status, rays_d, hit_slot2, grad2, rgb2, hit_slot, n_hit, S, w2b):
    """oi_bounce_resolve: status (S * n_hit,), rays_d (S * n_hit, 3), hit_slot2 (S * n_hit,), grad2 / rgb2 (n_hit2, 3) or None,
    hit_slot (N,) -> the bounce transfer (3, 9, N); the mean over a pixel's samples of [front-facing hit] rho A_Y_MAX (3, 9, N),
    which the bar scales with; n . d of every ray (S, n_hit) (0 where there is no hit) and the front-facing hits (S, n_hit)."""
    slot = np.asarray(hit_slot)
    N = len(slot)
    out, mag = np.zeros((3, E.N_COEFFS, N)), np.zeros((3, E.N_COEFFS, N))
    n2 = 0 if grad2 is None else len(grad2)
    if n_hit == 0 or n2 == 0:
        return out, mag, np.zeros((S, n_hit)), np.zeros((S, n_hit), dtype=bool)
    st = np.asarray(status).reshape(S, n_hit)
    k = np.asarray(hit_slot2).reshape(S, n_hit).astype(np.int64)
    d = np.asarray(rays_d, dtype=np.float64).reshape(S, n_hit, 3)
    ok = (st == T.HIT) & (k >= 0) & (k < n2)
    kk = np.where(ok, k, 0)
    g = np.asarray(grad2, dtype=np.float64)[kk]
    n = g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-6)
    nd = np.where(ok, (n * d).sum(-1), 0.0)
    front = ok & (nd < 0)
    t = E.closed_form(n @ np.asarray(w2b, dtype=np.float64)[:3, :3])              # (S, n_hit, 9): A_band y_c(W^T n)
    rho = np.asarray(rgb2, dtype=np.float64)[kk] * front[..., None]               # (S, n_hit, 3)
    b = np.einsum("jik,jic->ikc", rho, t) / S                                     # (n_hit, 3, 9)
    m = np.einsum("jik,c->ikc", np.abs(rho), A_Y_MAX) / S
    on = slot >= 0
    out[:, :, on] = b[slot[on]].transpose(1, 2, 0)
    mag[:, :, on] = m[slot[on]].transpose(1, 2, 0)
    return out, mag, nd, front


def resolve_bar(mag, S):
    """The bar of oi_bounce_resolve per output: (TERM_ROUNDINGS + S + 2) 2^-24 mag -- the roundings of a term, one for the fmaf
    that multiplies by rho and adds, S for the accumulation (each rounds a partial sum of magnitude <= S mag), one division."""
    return (TERM_ROUNDINGS[None, :, None] + S + 2.0) * EPS * mag


def shade(transfer_map, bounce, envs, mask, albedo, bg=None):
    """oi_env_shade_bounce: transfer (9, N), bounce (3, 9, N), envs (F, 9, 3), mask (N,) bool, albedo (N, 3) -> shading,
    indirect, image (F, 3, N), and sum_c (|T_c| + |B_c|) |env_c| (F, 3, N) the bar scales with."""
    t, b, e = (np.asarray(x, dtype=np.float64) for x in (transfer_map, bounce, envs))
    m = np.asarray(mask, dtype=bool)
    direct = np.einsum("qn,fqk->fkn", t, e) * m
    ind = np.einsum("kqn,fqk->fkn", b, e) * m
    mag = np.einsum("qn,fqk->fkn", np.abs(t), np.abs(e)) + np.einsum("kqn,fqk->fkn", np.abs(b), np.abs(e))
    sh = direct + ind
    bgv = np.zeros(3) if bg is None else np.asarray(bg, dtype=np.float64)
    img = np.where(m[None, None, :], np.maximum(sh, 0.0) * np.asarray(albedo, dtype=np.float64).T[None], bgv[None, :, None])
    return sh, ind, img, mag


# 18 fmafs (two chains of 9, each rounding a partial sum of magnitude <= mag) and one addition; the image has one product more
SHADE_ROUNDINGS = 19.0


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene: env_ref's two spheres, seen from the biased point on top of the lower one
# ---------------------------------------------------------------------------------------------------------------------
def blocker_hits(o, d):
    """Nearest intersection of rays (.., 3) + (.., 3) (unit directions) with the upper sphere of env_ref: -> hit (..,) bool, the
    ray parameter, the point and the outward unit normal (garbage where hit is False)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    oc = o - E.C1
    b = -(oc * d).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - E.R1 ** 2)
    hit = (disc > 0) & (b > 0)
    t = b - np.sqrt(np.maximum(disc, 0.0))
    y = o + t[..., None] * d
    return hit, t, y, (y - E.C1) / E.R1


def top_estimator(S, seed, pix, rho, bias=T.BIAS):
    """The S-sample estimator of the bounce transfer at the point on top of the lower sphere for the pixel numbers pix (n,),
    through resolve(): oi_occlusion_ambient_begin's directions, analytic intersections with the upper sphere, its analytic
    normals, the constant albedo rho (3,).  Object frame = world frame.  -> (3, 9, n) and the share of rays that hit."""
    pix = np.asarray(pix)
    n = len(pix)
    pts = np.tile([0.0, 0.0, E.R0], (n, 1))
    o, d, _, traced = R.ambient_rays(pts, pts / E.R0, pix, S, seed, bias, distance=4.0)
    hit, _, _, nrm = blocker_hits(o, d)
    hit &= traced
    status = np.where(hit, T.HIT, T.MISS).reshape(-1)
    slot2 = np.full(S * n, -1)
    slot2[hit.reshape(-1)] = np.arange(int(hit.sum()))
    grad2 = nrm.reshape(-1, 3)[hit.reshape(-1)]
    rgb2 = np.tile(np.asarray(rho, dtype=np.float64), (len(grad2), 1))
    out, _, _, front = resolve(status, d.reshape(-1, 3), slot2, grad2, rgb2, np.arange(n), n, S, np.eye(4))
    assert (front == hit).all()                    # a nearest intersection from outside is a front face
    return out, float(hit.mean())


def top_quadrature(bias=T.BIAS, n=200000):
    """The bounce transfer per unit albedo at that point, integral over the cap the upper sphere covers of
    A_band(c) y_c(n(w)) cos(theta) / pi dw with n(w) the sphere's normal where the ray towards w meets it: -> (9,).  By the
    symmetry about the axis only c = 0, 2, 6 are non-zero (the azimuth integral of the others vanishes); midpoint rule in theta
    in the manner of env_ref.cap_transfer."""
    alpha = E.analytic_cap_angle(bias)
    th = (np.arange(n) + 0.5) * alpha / n
    d = np.stack([np.sin(th), np.zeros(n), np.cos(th)], -1)
    hit, _, _, nrm = blocker_hits(np.array([0.0, 0.0, E.R0 + bias]), d)
    assert hit.all()
    t = E.closed_form(nrm)
    out = np.zeros(E.N_COEFFS)
    for c in (0, 2, 6):
        out[c] = (t[:, c] * np.cos(th) * np.sin(th)).sum() * (alpha / n) * 2.0
    return out


def standard_error_bar(S, rho):
    """5 standard errors of the S-sample estimator per coefficient, from the per-sample bound 0.5 rho A_band |y_c|max: (9,)."""
    return 5.0 * 0.5 * rho * A_Y_MAX / np.sqrt(S)
