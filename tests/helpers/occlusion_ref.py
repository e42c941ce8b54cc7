"""fp64 CPU restatement of include/oi_occlusion.h: the sample numbers, the tangent frame, the cap and
hemisphere directions, the soft-shadow and ambient-occlusion rays, the any-hit ray machine, the resolve rule and the shade
expression with an occlusion factor -- plus the views, lights and settings the CPU rehearsal and the GPU tests share.  Builds
on tests/helpers/trace_ref.py; nothing here touches the code under test."""
import numpy as np

from helpers import mesh_attr_ref as A
from helpers import trace_ref as T

MAX_SAMPLES = 256            # OI_OCCLUSION_MAX_SAMPLES

# the golden-field configuration of tests/test_gpu_occlusion.py, rehearsed on the oracle alone by tests/test_occlusion_cpu.py
R_SOFT = 24
SOFT_VIEWS = [(0, "centre"), (1, "off")]
SOFT_LIGHTS = T.LIGHT_DIRS[:2]
SOFT_RADIUS = 0.1            # radians
SOFT_S = 4
AO_S = 4
AO_DISTANCE = 0.5
SEED = 7
REHEARSAL_LIMIT_CAP = 0.01   # LIMIT share of the secondary rays on the oracle alone
LIMIT_CAP = 0.02             # ... and of the library's (twice the rehearsal's)

# the analytic two-sphere scene of the GPU tests: a large sphere at the origin, a small one above it on the light's axis
C0, R0 = np.array([0.0, 0.0, 0.0]), 0.5
C1, R1 = np.array([0.0, 0.0, 0.8]), 0.1
ANALYTIC_AXIS = (0.0, 0.0, 1.0)
ANALYTIC_RADIUS, ANALYTIC_S, ANALYTIC_PATCH = 0.15, 64, 16
TANGENCY_BAND = 1e-4
EXCLUDED_CAP = 0.01


def two_spheres(p):
    p = np.asarray(p, dtype=np.float64)
    return np.minimum(np.linalg.norm(p - C0, axis=-1) - R0, np.linalg.norm(p - C1, axis=-1) - R1)


def analytic_patch(n=ANALYTIC_PATCH, half=0.2):
    """n x n points on top of the large sphere (x, y in [-half, half]) and their normals.  -> points, normals (n*n, 3)."""
    g = np.linspace(-half, half, n)
    x, y = (v.reshape(-1) for v in np.meshgrid(g, g, indexing="xy"))
    z = np.sqrt(R0 * R0 - x * x - y * y)
    p = np.stack([x, y, z], -1)
    return p, p / R0


def mix(pix, seed):
    """The header's 32-bit mix of (pixel, seed): uint32, wrapping."""
    x = (np.asarray(pix).astype(np.uint64) * 0x9E3779B9 + int(seed)) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def sample_numbers(pix, seed, S):
    """u1 (S,), u2 (S, n) of samples 0 .. S-1 at the pixels pix (n,): the float32 numbers of the kernel, exactly, as float64."""
    j = np.arange(S)
    u1 = ((j.astype(np.float32) + np.float32(0.5)) / np.float32(S)).astype(np.float64)
    x = mix(pix, seed)
    u2 = (((j.astype(np.uint64)[:, None] * 2654435769 + x[None, :]) & 0xFFFFFFFF) >> 8).astype(np.float64) * 2.0 ** -24
    return u1, u2


def frame(a):
    """Duff et al. 2017: the tangent frame (t1, t2) of unit axes a (..., 3), without a branch."""
    a = np.asarray(a, dtype=np.float64)
    x, y, z = a[..., 0], a[..., 1], a[..., 2]
    sg = np.copysign(1.0, z)
    aa = -1.0 / (sg + z)
    b = x * y * aa
    t1 = np.stack([1.0 + sg * x * x * aa, sg * b, -sg * x], -1)
    t2 = np.stack([b, sg + y * y * aa, -y], -1)
    return t1, t2


def directions(a, sin_a, cos_a, u2):
    """d = sin(alpha) cos(phi) t1 + sin(alpha) sin(phi) t2 + cos(alpha) a, phi = 2 pi u2; a (..., 3), the rest (...)."""
    t1, t2 = frame(a)
    phi = 2.0 * np.pi * np.asarray(u2, dtype=np.float64)
    e1, e2 = (sin_a * np.cos(phi))[..., None], (sin_a * np.sin(phi))[..., None]
    return e1 * t1 + e2 * t2 + np.asarray(cos_a, dtype=np.float64)[..., None] * np.asarray(a, dtype=np.float64)


def clamp_radius(radius):
    r = np.float64(radius)
    return 0.0 if np.isnan(r) else float(min(max(r, 0.0), np.pi / 2))


def cap_directions(l, radius, u1, u2):
    """Uniform in solid angle over the cap of angular radius `radius` about the unit vector l: u1 (S,), u2 (S, n) -> (S, n, 3)."""
    cos_a = 1.0 - u1 * (1.0 - np.cos(clamp_radius(radius)))
    sin_a = np.sqrt(np.maximum(0.0, 1.0 - cos_a * cos_a))
    S, n = u2.shape
    return directions(np.broadcast_to(l, (S, n, 3)), np.broadcast_to(sin_a[:, None], (S, n)), np.broadcast_to(cos_a[:, None], (S, n)), u2)


def hemisphere_directions(normals, u1, u2):
    """Cosine-weighted over the hemisphere about each unit normal (n, 3): -> (S, n, 3)."""
    S, n = u2.shape
    cos_a, sin_a = np.sqrt(1.0 - u1), np.sqrt(u1)
    return directions(np.broadcast_to(normals, (S, n, 3)), np.broadcast_to(sin_a[:, None], (S, n)), np.broadcast_to(cos_a[:, None], (S, n)), u2)


def unit_sphere_exit(o, d):
    b, c = (o * d).sum(-1), (o * o).sum(-1) - 1.0
    disc = b * b - c
    return np.where(disc > 0, np.maximum(np.sqrt(np.maximum(disc, 0.0)) - b, 0.0), 0.0)


def _rays(points, normals, d, bias):
    S, n = d.shape[:2]
    o = np.broadcast_to(np.asarray(points, dtype=np.float64) + bias * normals, (S, n, 3))
    return o, unit_sphere_exit(o, d), (normals[None] * d).sum(-1) > 0


def light_rays(points, grad, pix, l, radius, S, seed, bias=T.BIAS):
    """oi_occlusion_light_begin for one light of object-frame direction l: -> origins, directions (S, n, 3), far, traced (S, n)."""
    normals = A.unit(np.asarray(grad, dtype=np.float64))
    u1, u2 = sample_numbers(pix, seed, S)
    d = cap_directions(np.asarray(l, dtype=np.float64), radius, u1, u2)
    o, far, traced = _rays(points, normals, d, bias)
    return o, d, far, traced


def ambient_rays(points, grad, pix, S, seed, bias=T.BIAS, distance=AO_DISTANCE):
    """oi_occlusion_ambient_begin: -> origins, directions (S, n, 3), far, traced (S, n)."""
    normals = A.unit(np.asarray(grad, dtype=np.float64))
    u1, u2 = sample_numbers(pix, seed, S)
    d = hemisphere_directions(normals, u1, u2)
    o, far, traced = _rays(points, normals, d, bias)
    return o, d, np.minimum(far, distance), traced


def trace_anyhit(sdf_fn, o, d, near, far, tol=T.TOL, omega=T.OMEGA, max_steps=T.MAX_STEPS):
    """The state machine of oi_occlusion_step in float64, all rays in lock step: T.trace's MARCH phase, and a later negative
    sample ends the ray as a HIT at that sample.  -> t, status (uint8), steps, rays in flight before each step."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    N = len(o)
    t = np.array(near, dtype=np.float64).reshape(N).copy()
    far = np.asarray(far, dtype=np.float64).reshape(N)
    status = np.full(N, T.MARCH, dtype=np.uint8)
    steps = np.zeros(N, dtype=np.int64)
    in_flight = []
    for _ in range(max_steps):
        act = np.nonzero(status == T.MARCH)[0]
        if len(act) == 0:
            break
        in_flight.append(len(act))
        s = np.asarray(sdf_fn(o[act] + t[act, None] * d[act]), dtype=np.float64)
        steps[act] += 1
        bad = ~np.isfinite(s)
        hit = ~bad & (np.abs(s) <= tol)
        pos = ~bad & ~hit & (s > 0)
        neg = ~bad & ~hit & ~pos
        status[act[bad]] = T.NONFINITE
        status[act[hit]] = T.HIT
        status[act[neg]] = np.where(steps[act[neg]] == 1, T.START_INSIDE, T.HIT)
        tn = t[act[pos]] + np.maximum(omega * s[pos], tol)
        t[act[pos]] = tn
        status[act[pos][tn > far[act[pos]]]] = T.MISS
    status[status >= T.MARCH] = T.LIMIT
    return t, status, steps, in_flight


def resolve(status, hit_slot, n_hit, L, S):
    """oi_occlusion_resolve: status (L * S * n_hit,), hit_slot (N,) -> (L, N): MISS count / S at the hit's slot, 1 off the mask."""
    st = np.asarray(status).reshape(L, S, n_hit)
    slot = np.asarray(hit_slot)
    out = np.ones((L, len(slot)), dtype=np.float64)
    share = ((st == T.MISS).sum(1).astype(np.float32) / np.float32(S)).astype(np.float64)
    out[:, slot >= 0] = share[:, slot[slot >= 0]]
    return out


def shade(ro, rd, t, grad, rgb, w2b, lights, visibility=None, ao=None):
    """oi_surface_shade_ao on hit rays, float64: (ao ambient + vis diffuse) albedo + vis specular -> (L, 3, n)."""
    n, L = len(t), np.asarray(lights).reshape(-1, 16).shape[0]
    full = T.shade(ro, rd, t, grad, rgb, w2b, lights, visibility=np.ones((L, n)))
    amb = T.shade(ro, rd, t, grad, rgb, w2b, lights, visibility=np.zeros((L, n)))
    vis = np.ones((L, n)) if visibility is None else np.asarray(visibility, dtype=np.float64)
    occ = np.ones(n) if ao is None else np.asarray(ao, dtype=np.float64)
    return occ[None, None, :] * amb + vis[:, None, :] * (full - amb)


def closest_approach(o, d, far, c=C1):
    """Distance from c to the closest point of each segment o + t d, 0 <= t <= far."""
    tc = np.clip(((c - o) * d).sum(-1), 0.0, far)
    return np.linalg.norm(o + tc[..., None] * d - c, axis=-1)


def rehearse_soft(seed, pose_name, R=R_SOFT):
    """The secondary rays of one golden view on the oracle alone, at the settings above: the oracle's own primary trace, then
    soft-shadow rays under SOFT_LIGHTS and ambient-occlusion rays through the any-hit machine.  -> dict of counts."""
    fld = T.Field(seed)
    ro, rd, near, far, w2b = T.view_rays(pose_name, R)
    t, status, _, _ = T.trace(fld.sdf, ro, rd, near, far)
    hit = status == T.HIT
    pix = np.nonzero(hit)[0]
    pts = ro[hit] + t[hit, None] * rd[hit]
    _, g, _ = fld.full(pts)
    out = {"n_hit": int(hit.sum())}
    sets = {f"light{i}": light_rays(pts, g, pix, T.light_object_dir(dd, w2b), SOFT_RADIUS, SOFT_S, SEED) for i, dd in enumerate(SOFT_LIGHTS)}
    sets["ambient"] = ambient_rays(pts, g, pix, AO_S, SEED)
    for name, (o, d, sfar, traced) in sets.items():
        m = traced.reshape(-1)
        _, st, _, in_flight = trace_anyhit(fld.sdf, o.reshape(-1, 3)[m], d.reshape(-1, 3)[m], np.zeros(int(m.sum())), sfar.reshape(-1)[m])
        out[name] = {"traced": int(m.sum()), "of": int(m.size), "limit": int((st == T.LIMIT).sum()),
                     "start_inside": int((st == T.START_INSIDE).sum()), "occluded": int((st == T.HIT).sum()),
                     "lit": int((st == T.MISS).sum()), "evals": int(sum(in_flight))}
    return out
