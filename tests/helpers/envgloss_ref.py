"""fp64 numpy restatement of include/oi_envgloss.h, written from the header: the Phong-lobe prefilter
of an equirectangular map, the reflection-lobe sampler and its rays, the rotated bilinear lookup and the glossy shading --
plus the reflection-lobe visibility of tests/helpers/env_ref.py's analytic two-sphere scene, integrated in float64.
Builds on env_ref.py (pixel directions and weights, the SH shading) and occlusion_ref.py (sample numbers, tangent frame,
direction formula); nothing here touches the code under test."""
import numpy as np

from helpers import env_ref as E
from helpers import occlusion_ref as R

MIN_SHININESS, MAX_SHININESS = 1.0, 4096.0     # OI_ENVGLOSS_MIN_SHININESS / _MAX_SHININESS
CHUNK, TILE = 2048, 256                        # OI_ENVGLOSS_CHUNK; the output texels of one workgroup
ANALYTIC_BIAS = 1e-3                           # the analytic scene's offset along the normal


def lobe(x, s):
    """K(x) = x^s for x > 0, an exact 0 otherwise."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0, np.power(np.maximum(x, 1e-300), s), 0.0)


def convolve(radiance, s, d):
    """G_s of the maps radiance (E, 3, He, We) towards unit vectors d (n, 3), the header's sum over the input pixels:
    -> G (E, 3, n); the sums of (w / pi) |L| K the bar scales with; and the sums of (w / pi) |L| s x^(s - 1) [x > 0], the
    sensitivity of G to an error of the cosine x."""
    L = np.asarray(radiance, dtype=np.float64)
    d_in, w = E.equirect(*L.shape[2:])
    x = np.einsum("nk,rck->nrc", np.asarray(d, dtype=np.float64), d_in)
    wk = (w[None, :, None] / np.pi) * lobe(x, s)
    wd = (w[None, :, None] / np.pi) * np.where(x > 0, s * np.power(np.maximum(x, 1e-300), s - 1.0), 0.0)
    return np.einsum("nrc,ekrc->ekn", wk, L), np.einsum("nrc,ekrc->ekn", wk, np.abs(L)), np.einsum("nrc,ekrc->ekn", wd, np.abs(L))


def prefilter(radiance, s, Hp, Wp):
    """oi_env_prefilter: radiance (E, 3, He, We) -> glossy (E, 3, Hp, Wp), and convolve's two magnitudes in that shape."""
    d_out, _ = E.equirect(Hp, Wp)
    return tuple(v.reshape(v.shape[0], 3, Hp, Wp) for v in convolve(radiance, s, d_out.reshape(-1, 3)))


def prefilter_rounding_sigma(radiance, s, Hp, Wp):
    """The standard deviation of oi_env_prefilter's float32 result about the exact sum, in units of 2^-24, per output value
    (E, 3, Hp, Wp): first-order propagation of independent rounding errors, each uniform within its bound (half an ulp for an
    operation, one ulp for sincospif, v_log_f32 and v_exp_f32), through the header's expressions and its order of summation.
    With a_p = (w / pi) L K(x_p) and b_p = (w / pi) L s x_p^(s - 1) the signed terms and their derivatives by the cosine:

      the output texel's direction   |sum_p b_p d_p|^2 v_o      one error for every term: it adds coherently
      the input texels' directions   sum_p b_p^2 (v_p + 1)      and the three roundings of the dot product
      the records and the lobe       sum_p a_p^2 (4 + 0.8 e_p^2),   e_p = s log2 x_p: the error of the exponent scales with it
      the additions                  sum over every partial sum of the two stages of its square / 3

    v = (theta^2 + phi^2 sin^2 theta) / 3 + 3 is the variance of a texel's direction: the float32 arguments of sincospif carry
    a relative half-ulp, i.e. angle errors of up to theta and phi units, its two results an ulp each, their product half."""
    L = np.asarray(radiance, dtype=np.float64)
    n_env, _, He, We = L.shape
    P, O = He * We, Hp * Wp
    d_in, w = E.equirect(He, We)
    d_out, _ = E.equirect(Hp, Wp)
    d_in, d_out = d_in.reshape(P, 3), d_out.reshape(O, 3)

    def var_dir(H, W):
        th = (np.pi * (np.arange(H) + 0.5) / H)[:, None]
        ph = (2.0 * np.pi * (np.arange(W) + 0.5) / W)[None, :]
        return ((th ** 2 + (ph * np.sin(th)) ** 2) / 3.0 + 3.0).reshape(-1)

    v_in, v_out = var_dir(He, We), var_dir(Hp, Wp)
    x = d_out @ d_in.T                                               # (O, P)
    pos = x > 0
    xs = np.where(pos, x, 1.0)
    wl = (np.repeat(w, We)[None, None, :] / np.pi) * L.reshape(n_env, 3, P)        # (E, 3, P)
    a = wl[:, :, None, :] * np.where(pos, xs ** s, 0.0)                             # (E, 3, O, P)
    b = wl[:, :, None, :] * np.where(pos, s * xs ** (s - 1.0), 0.0)
    e2 = np.where(pos, (s * np.log2(xs)) ** 2, 0.0)
    var = (np.einsum("ekop,pj->ekoj", b, d_in) ** 2).sum(-1) * v_out[None, None, :]
    var += (b ** 2 * (v_in + 1.0)).sum(-1) + (a ** 2 * (4.0 + 0.8 * e2)).sum(-1)
    # the additions, in the kernel's order: chains of 32 within batches of 256 within chunks of CHUNK, then the chunks
    nb = -(-P // CHUNK)
    assert nb <= 32, "stage 2 is one chain here"
    t = np.zeros(a.shape[:3] + (nb * CHUNK,))
    t[..., :P] = a
    t = t.reshape(a.shape[:3] + (nb, CHUNK // 256, 8, 32))
    for _ in range(4):                                               # chain, group, batch, chunk: the last axis each time
        c = np.cumsum(t, axis=-1)
        var += (c ** 2).sum(axis=tuple(range(3, c.ndim))) / 3.0
        t = c[..., -1]
    return np.sqrt(var).reshape(n_env, 3, Hp, Wp)


def lobe_angles(u1, s):
    """cos(alpha) = u1^(1 / (s + 1)), sin(alpha) = sqrt(max(0, 1 - cos^2)): density proportional to cos^s over the lobe."""
    c = np.power(np.asarray(u1, dtype=np.float64), 1.0 / (s + 1.0))
    return c, np.sqrt(np.maximum(0.0, 1.0 - c * c))


def _unit(v, eps=1e-6):
    v = np.asarray(v, dtype=np.float64)
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), eps)


def reflect(grad, points, eyes):
    """n = g / max(|g|, 1e-6), v = (eye - point) / max(|.|, 1e-6), r = 2 (n . v) n - v: each (n, 3)."""
    n, v = _unit(grad), _unit(np.asarray(eyes, dtype=np.float64) - np.asarray(points, dtype=np.float64))
    return n, v, 2.0 * (n * v).sum(-1, keepdims=True) * n - v


def lobe_directions(axes, pix, S, s, seed):
    """The S sample directions about each axis (n, 3) at the pixels pix (n,): -> (S, n, 3)."""
    u1, u2 = R.sample_numbers(pix, seed, S)
    c, sn = lobe_angles(u1, s)
    n = len(pix)
    return R.directions(np.broadcast_to(axes, (S, n, 3)), np.broadcast_to(sn[:, None], (S, n)), np.broadcast_to(c[:, None], (S, n)), u2)


def lobe_rays(points, grad, pix, eyes, S, s, seed, bias):
    """oi_occlusion_lobe_begin; eyes (n, 3) = rays_o[pix].  -> origins, directions (S, n, 3), far, traced, n . d (S, n)."""
    n, _, r = reflect(grad, points, eyes)
    d = lobe_directions(r, pix, S, s, seed)
    o = np.broadcast_to(np.asarray(points, dtype=np.float64) + bias * n, d.shape)
    nd = (n[None] * d).sum(-1)
    return o, d, R.unit_sphere_exit(o, d), nd > 0, nd


def lookup_coords(d, Hp, Wp):
    """The continuous texel coordinates (u, v) of unit vectors d (..., 3)."""
    d = np.asarray(d, dtype=np.float64)
    theta = np.arccos(np.clip(d[..., 2], -1.0, 1.0))
    phi = np.arctan2(d[..., 1], d[..., 0])
    phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
    return theta / np.pi * Hp - 0.5, phi / (2.0 * np.pi) * Wp - 0.5


def bilinear(g, u, v):
    """g (3, Hp, Wp) at coordinates (u, v) (...): rows clamped, columns modulo Wp.  -> (..., 3)."""
    g = np.asarray(g, dtype=np.float64)
    Hp, Wp = g.shape[1:]
    i0, j0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = (u - i0)[..., None], (v - j0)[..., None]
    ia, ib = np.clip(i0, 0, Hp - 1), np.clip(i0 + 1, 0, Hp - 1)
    ja, jb = np.mod(j0, Wp), np.mod(j0 + 1, Wp)
    at = lambda i, j: np.moveaxis(g[:, i, j], 0, -1)
    top = (1 - fv) * at(ia, ja) + fv * at(ia, jb)
    bot = (1 - fv) * at(ib, ja) + fv * at(ib, jb)
    return (1 - fu) * top + fu * bot


def adjacent_difference(g):
    """The largest difference between texels that one bilinear cell joins (rows clamped, columns wrapped), per channel (3,)."""
    g = np.asarray(g, dtype=np.float64)
    dj = np.abs(g - np.roll(g, -1, axis=2)).max((1, 2))
    di = np.abs(g[:, 1:] - g[:, :-1]).max((1, 2)) if g.shape[1] > 1 else np.zeros(3)
    return np.maximum(di, dj)


def lookup(g, d):
    return bilinear(g, *lookup_coords(d, *np.asarray(g).shape[1:]))


def lookup_directions(grad, points, eyes, w2b, rot):
    """The lookup direction of every environment at every hit: R_f^T w2b[:3,:3]^T r -> (F, n, 3)."""
    _, _, r = reflect(grad, points, eyes)
    rw = r @ np.asarray(w2b, dtype=np.float64)[:3, :3]            # row k: W^T r_k
    return np.einsum("nk,fkj->fnj", rw, np.asarray(rot, dtype=np.float64))   # row: R_f^T r_w


def shade_glossy(transfer_map, envs, mask, slot, albedo, grad, points, eyes, w2b, spec_vis, maps, map_index, rot, k_s, bg=None):
    """oi_env_shade_glossy.  transfer (9, N), envs (F, 9, 3), mask (N,), slot (N,) the hit slots, albedo (N, 3), grad / points
    (n_hit, 3), eyes (N, 3), spec_vis (N,) or None, maps (M, 3, Hp, Wp), rot (F, 3, 3), k_s (3,).
    -> shading, image, specular (F, 3, N), the diffuse magnitude sum |T env| and the lookups (F, 3, N) (0 off the mask)."""
    sh, img, mag = E.shade(transfer_map, envs, mask, albedo, bg)
    F, N = len(envs), len(mask)
    look = np.zeros((F, 3, N))
    m = np.asarray(mask, dtype=bool)
    if m.any():
        k = np.asarray(slot)[m]
        d = lookup_directions(np.asarray(grad)[k], np.asarray(points)[k], np.asarray(eyes)[m], w2b, rot)
        for f in range(F):
            look[f][:, m] = lookup(np.asarray(maps)[map_index[f]], d[f]).T
    vis = np.ones(N) if spec_vis is None else np.asarray(spec_vis, dtype=np.float64)
    spec = np.asarray(k_s, dtype=np.float64)[None, :, None] * vis[None, None, :] * look
    img = np.where(m[None, None, :], img + spec, img)
    return sh, img, spec, mag, look


def lobe_test_inputs(rs, n_hit, n_primary):
    """Inputs of oi_occlusion_lobe_begin for the GPU tests: hit points inside the unit ball, gradients of any length, and eyes
    from head-on to grazing -- the reflected vector makes 0 .. 1.3 rad with the normal, so the broad lobes cross the horizon
    and the narrow ones do not.  -> points, grad (n_hit, 3), pix (n_hit,), eyes (n_primary, 3) with the hits' eyes at pix; float32."""
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    pts = (0.5 * unit(rs.randn(n_hit, 3)) * rs.uniform(0.2, 1.0, (n_hit, 1))).astype(np.float32)
    grad = (unit(rs.randn(n_hit, 3)) * rs.uniform(0.3, 3.0, (n_hit, 1))).astype(np.float32)
    n = unit(grad.astype(np.float64))
    tang = unit(np.cross(n, rs.randn(n_hit, 3)))
    beta = rs.uniform(0.0, 1.3, (n_hit, 1))
    v = np.cos(beta) * n + np.sin(beta) * tang
    pix = rs.permutation(n_primary)[:n_hit]
    eyes = np.zeros((n_primary, 3), dtype=np.float32)
    eyes[pix] = (pts + v * rs.uniform(1.5, 3.0, (n_hit, 1))).astype(np.float32)
    return pts, grad, pix, eyes


LOBE_CASES = [(n_hit, S, s) for n_hit in (1, 65, 130) for S in (1, 3, 256) for s in (1, 10, 200)]


def lobe_case(n_hit, S, s):
    """The inputs of one case of tests/test_gpu_envgloss.py::test_lobe_begin (its seed is 11 + s)."""
    return lobe_test_inputs(np.random.RandomState(n_hit * 1000 + S * 10 + s), n_hit, 2 * n_hit + 3)


def analytic_eye(beta, distance=2.0):
    """The eye from which the reflected view vector at the top of the analytic scene's lower sphere makes the angle beta with
    the normal (+z), in the x-z plane: v is r mirrored about n."""
    return np.array([0.0, 0.0, E.R0]) + distance * np.array([-np.sin(beta), 0.0, np.cos(beta)])


def analytic_lobe_visibility(beta, s, bias=ANALYTIC_BIAS, n1=2000, n2=2000):
    """V_spec at the top of the lower sphere of the analytic scene for a reflected view vector at angle beta to the normal:
    the share of the lobe cos^s about r that is above the horizon and misses the upper sphere, by the midpoint rule over the
    sampler's own (u1, u2) square (uniform in the lobe's measure)."""
    u1 = (np.arange(n1) + 0.5) / n1
    u2 = (np.arange(n2) + 0.5) / n2
    c, sn = lobe_angles(u1, s)
    r = np.array([np.sin(beta), 0.0, np.cos(beta)])
    d = R.directions(np.broadcast_to(r, (n1, n2, 3)), np.broadcast_to(sn[:, None], (n1, n2)), np.broadcast_to(c[:, None], (n1, n2)),
                     np.broadcast_to(u2[None, :], (n1, n2)))
    o = np.array([0.0, 0.0, E.R0 + bias])
    oc = E.C1 - o
    tc = d @ oc                                                   # closest approach to the upper sphere's centre
    dist2 = (oc * oc).sum() - tc * tc
    blocked = (tc > 0) & (dist2 < E.R1 * E.R1)
    return float(((d[..., 2] > 0) & ~blocked).mean())
