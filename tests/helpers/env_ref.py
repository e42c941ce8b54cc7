"""fp64 numpy restatement of include/oi_envlight.h: the SH basis, the equirectangular projection, the
sample directions (tests/helpers/occlusion_ref.py's sample numbers and hemisphere), the transfer estimator, the unshadowed
closed form, the shading and the SH rotation -- plus the analytic two-sphere scene of the GPU test and its cap integral.
Nothing here touches the code under test."""
import numpy as np

from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T

N_COEFFS = 9
BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
A_HAT = np.array([1.0, 2.0 / 3.0, 0.25])          # the clamped-cosine kernel per band, divided by pi
MAX_ENVS = 256                                    # OI_ENV_MAX_ENVS
PROJECT_CHUNK = 8192                              # pixels per partial of oi_env_project
Y_MAX_BAND1 = np.sqrt(3.0 / (4.0 * np.pi))        # |y1..3| <= 0.4886

# the analytic scene of tests/test_gpu_envlight.py: a sphere at the origin and a larger-looking one above it on the z axis,
# both inside the unit ball.  From the biased point on top of the lower sphere the upper one covers a cap of half-angle
# asin(R1 / (C1z - R0 - bias)) = asin(0.25 / 0.34) = 0.826 rad about the normal.
C0, R0 = np.array([0.0, 0.0, 0.0]), 0.3
C1, R1 = np.array([0.0, 0.0, 0.65]), 0.25


def basis(d):
    """The header's basis at unit vectors d (..., 3) -> (..., 9); the constants in full precision."""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k1, k2 = np.sqrt(3.0 / (4.0 * np.pi)), np.sqrt(15.0 / (4.0 * np.pi))
    return np.stack([np.full_like(x, 0.5 / np.sqrt(np.pi)), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z,
                     np.sqrt(5.0 / (16.0 * np.pi)) * (3.0 * z * z - 1.0), k2 * x * z, np.sqrt(15.0 / (16.0 * np.pi)) * (x * x - y * y)], -1)


def sinpi(x):
    """sin(pi x), exact at the multiples of 1/2 (np.sin(np.pi) is 1.2e-16: a map of one pixel has its centre there, and
    an error bar relative to sum |w L y| leaves no room for it)."""
    x = np.mod(np.asarray(x, dtype=np.float64), 2.0)
    sign = np.where(x > 1.0, -1.0, 1.0)
    x = np.where(x > 1.0, x - 1.0, x)
    return sign * np.sin(np.pi * np.where(x > 0.5, 1.0 - x, x))


def cospi(x):
    return sinpi(np.asarray(x, dtype=np.float64) + 0.5)


def equirect(He, We):
    """Directions (He, We, 3) and weights (He,) of the header's equirectangular pixels."""
    r, c = np.arange(He, dtype=np.float64), np.arange(We, dtype=np.float64)
    theta, phi = (r + 0.5) / He, 2.0 * (c + 0.5) / We                          # in units of pi
    d = np.stack([sinpi(theta)[:, None] * cospi(phi)[None, :], sinpi(theta)[:, None] * sinpi(phi)[None, :],
                  np.broadcast_to(cospi(theta)[:, None], (He, We))], -1)
    w = (np.cos(np.pi * r / He) - np.cos(np.pi * (r + 1.0) / He)) * 2.0 * np.pi / We
    return d, w


def project(radiance):
    """oi_env_project: radiance (E, 3, He, We) -> coefficients (E, 9, 3) and the sums of |w L y| (E, 9, 3) the bar scales with."""
    L = np.asarray(radiance, dtype=np.float64)
    d, w = equirect(L.shape[2], L.shape[3])
    wy = w[:, None, None] * basis(d)                                  # (He, We, 9)
    return np.einsum("rcq,ekrc->eqk", wy, L), np.einsum("rcq,ekrc->eqk", np.abs(wy), np.abs(L))


def world_directions(rays_d, w2b):
    """d_w = normalize(w2b[:3,:3]^T d, eps 1e-6)."""
    v = np.asarray(rays_d, dtype=np.float64) @ np.asarray(w2b, dtype=np.float64)[:3, :3]   # row q: W^T d_q
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-6)


def transfer(status, rays_d, hit_slot, n_hit, S, w2b):
    """oi_transfer_resolve: status (S * n_hit,), rays_d (S * n_hit, 3), hit_slot (N,) -> (9, N)."""
    slot = np.asarray(hit_slot)
    out = np.zeros((N_COEFFS, len(slot)))
    if n_hit == 0:
        return out
    esc = (np.asarray(status).reshape(S, n_hit) == T.MISS)[..., None]
    y = basis(world_directions(np.asarray(rays_d).reshape(S, n_hit, 3), w2b))
    t = (esc * y).sum(0) / S                                          # (n_hit, 9)
    out[:, slot >= 0] = t[slot[slot >= 0]].T
    return out


def closed_form(n_world):
    """The unshadowed transfer A_band y_c(n) of unit normals (..., 3) -> (..., 9)."""
    return A_HAT[BAND] * basis(n_world)


def transfer_normal(grad, hit_slot, w2b):
    """oi_transfer_normal: grad (n_hit, 3), hit_slot (N,) -> (9, N)."""
    slot = np.asarray(hit_slot)
    out = np.zeros((N_COEFFS, len(slot)))
    if len(grad):
        g = np.asarray(grad, dtype=np.float64)
        n = g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-6)
        t = closed_form(n @ np.asarray(w2b, dtype=np.float64)[:3, :3])
        out[:, slot >= 0] = t[slot[slot >= 0]].T
    return out


def sample_directions(normals, pix, S, seed):
    """The directions of oi_occlusion_ambient_begin's rays about unit normals (n, 3) at pixels pix (n,): -> (S, n, 3)."""
    u1, u2 = R.sample_numbers(pix, seed, S)
    return R.hemisphere_directions(np.asarray(normals, dtype=np.float64), u1, u2)


def estimate_all_escaped(normals, pix, S, seed):
    """The transfer estimator with every ray escaped, object frame = world frame: -> (n, 9)."""
    return basis(sample_directions(normals, pix, S, seed)).mean(0)


def shade(transfer_map, envs, mask, albedo, bg=None):
    """oi_env_shade: transfer (9, N), envs (F, 9, 3), mask (N,) bool, albedo (N, 3) (rows off the mask ignored)
    -> shading (F, 3, N), image (F, 3, N), and sum_c |T_c env_c| (F, 3, N) the bar scales with."""
    t, e = np.asarray(transfer_map, dtype=np.float64), np.asarray(envs, dtype=np.float64)
    m = np.asarray(mask, dtype=bool)
    sh = np.einsum("qn,fqk->fkn", t, e) * m
    mag = np.einsum("qn,fqk->fkn", np.abs(t), np.abs(e))
    b = np.zeros(3) if bg is None else np.asarray(bg, dtype=np.float64)
    img = np.where(m[None, None, :], np.maximum(sh, 0.0) * np.asarray(albedo, dtype=np.float64).T[None], b[None, :, None])
    return sh, img, mag


def rotation(Rm, seed=0, n=64):
    """The 9 x 9 SH rotation M of f'(d) = f(R^T d): coefficients' = M coefficients.  One dense least-squares solve over n
    seeded random directions (independent of the code under test, which solves per band on a fixed lattice)."""
    rs = np.random.RandomState(seed)
    d = A.unit(rs.randn(n, 3))
    return np.linalg.lstsq(basis(d), basis(d @ np.asarray(Rm, dtype=np.float64)), rcond=None)[0]


def axis_rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def random_rotation(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, [1, 0, 2]]


def cap_transfer(alpha, n=200000):
    """The part of the transfer a blocker covering the cap of half-angle alpha about the normal removes, in the frame whose z
    axis is the normal: integral over the cap of y_c(w) cos(theta) / pi dw -> (9,) (the non-zonal terms vanish), midpoint rule
    in theta."""
    th = (np.arange(n) + 0.5) * alpha / n
    zonal = basis(np.stack([np.sin(th), np.zeros(n), np.cos(th)], -1))
    out = np.zeros(N_COEFFS)
    for c in (0, 2, 6):   # the azimuth integral of the others is zero
        out[c] = (zonal[:, c] * np.cos(th) * np.sin(th)).sum() * (alpha / n) * 2.0
    return out


def two_spheres(p):
    p = np.asarray(p, dtype=np.float64)
    return np.minimum(np.linalg.norm(p - C0, axis=-1) - R0, np.linalg.norm(p - C1, axis=-1) - R1)


def analytic_cap_angle(bias=T.BIAS):
    """Half-angle of the upper sphere seen from the biased point on top of the lower one."""
    return float(np.arcsin(R1 / (C1[2] - R0 - bias)))
