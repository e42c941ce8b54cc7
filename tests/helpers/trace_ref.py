"""fp64 CPU restatement of the sphere tracer (include/oi_trace.h) on the oracle's field
(oracle/oi_oracle.py): the ray state machine, the shadow-ray set-up, the visibility rule and the shading (through
tests/helpers/relight_ref.py), plus the views, lights and checks the CPU rehearsal and the GPU tests share.  Nothing here
touches the code under test."""
import numpy as np
import torch

import oi_oracle as O
from helpers import mesh_attr_ref as A
from helpers.relight_ref import relight_ref

MISS, HIT, LIMIT, START_INSIDE, NONFINITE, BACKFACING = 0, 1, 2, 3, 4, 5     # OI_TRACE_* of include/oi_trace.h
MARCH, REFINE = 16, 17
TOL, OMEGA, MAX_STEPS, BIAS = 1e-5, 1.0, 64, 1e-2                             # OI_TRACE_DEFAULT_*
MAX_MAX_STEPS, COUNT_WORDS = 1024, 1026

# the caps the reference itself must satisfy on the test views (tests/test_trace_cpu.py) and the GPU tests then assert
LIMIT_CAP = 0.02              # share of primary rays still in flight after MAX_STEPS
SHADOW_START_INSIDE_CAP = 0.01
SEGMENT_SAMPLES = 128         # uniform oracle samples per ray segment
SEGMENT_BACKOFF = 2e-3        # hits are checked on [near, t - 2e-3]

# the test views: seeded latents 0, 1, 2 x two poses of the 48 x 48 example camera (fov 10 degrees); `off` is the first pose
# of tests/golden/f5_generator.npz (the object 5.8 units off the scene's centre), `centre` the second one's rotation at the
# centre
R_VIEW = 48
SEEDS = (0, 1, 2)
POSES = ("centre", "off")
VIEWS = [(s, p) for s in SEEDS for p in POSES]
# world-frame light directions (the light is directional: the vector points from the surface TO the light)
LIGHT_DIRS = ((0.3, -0.8, -0.5), (-0.7, -0.3, -0.6), (0.2, 0.9, -0.4))


def pose(name):
    with np.load(A.GOLDEN + "/f5_generator.npz") as g:
        b2w = torch.from_numpy(np.asarray(g["b2w"])).float()
    if name == "off":
        return b2w[0].clone()
    m = b2w[1].clone()
    m[:3, 3] = 0.0
    return m


def example_camera(R):
    """tests/test_gpu_modules.py::example_cfg."""
    fov, img, img_scene = 10.0, 256, 1588
    cam_dist = float(1 / np.tan(0.5 * fov * np.pi / 180))
    scene_fov = float(2 * np.arctan(img_scene / img * np.tan(0.5 * fov * np.pi / 180)) * 180 / np.pi)
    return cam_dist, scene_fov, int(R * img_scene / img)


def view_rays(pose_name, R=R_VIEW):
    """The oracle's rays of a view: rays_o, rays_d (N, 3), near, far (N,), w2b (4, 4), float64 numpy."""
    cam_dist, scene_fov, scene_res = example_camera(R)
    _, K_inv, c2w, w2c = O.camera_matrices(cam_dist, scene_fov, scene_res)
    ro, rd, _, w2b = O.gen_rays(pose(pose_name)[None], K_inv, c2w, w2c, cam_dist, R, scene_res)
    ro, rd = ro.reshape(-1, 3).double(), rd.reshape(-1, 3).double()
    near, far = O.near_far_from_sphere(ro, rd)
    return ro.numpy(), rd.numpy(), near.reshape(-1).numpy(), far.reshape(-1).numpy(), w2b[0].double().numpy()


class Field:
    """The oracle's field of the seeded latent on the golden weights."""
    _sd = None

    def __init__(self, seed):
        if Field._sd is None:
            Field._sd = A.golden_state()
        self.sd, self.csd = Field._sd
        self.w = O.style_mlp(self.sd, A.latent(seed).double())

    def sdf(self, pts, chunk=1 << 16):
        pts = torch.as_tensor(np.asarray(pts), dtype=torch.float64).reshape(-1, 3)
        out = []
        with torch.no_grad():
            for i in range(0, len(pts), chunk):
                out.append(O.sdf_forward(self.sd, pts[i:i + chunk], self.w)[0].squeeze(-1))
        return torch.cat(out).numpy() if out else np.zeros(0)

    def full(self, pts):
        """sdf (n,), gradient (n, 3), albedo (n, 3)."""
        return A.field(self.sd, self.csd, self.w, pts)


def trace(sdf_fn, o, d, near, far, tol=TOL, omega=OMEGA, max_steps=MAX_STEPS):
    """The state machine of oi_trace_step in float64, all rays in lock step.  -> t, status (uint8), steps (int), and the
    number of rays in flight before each step (its sum = the sdf evaluations a tracer with a fresh count needs)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    N = len(o)
    t = np.array(near, dtype=np.float64).reshape(N).copy()
    far = np.asarray(far, dtype=np.float64).reshape(N)
    status = np.full(N, MARCH, dtype=np.uint8)
    steps = np.zeros(N, dtype=np.int64)
    t_lo, s_lo, t_hi, s_hi = t.copy(), np.zeros(N), t.copy(), np.zeros(N)
    side = np.zeros(N, dtype=np.int64)
    in_flight = []
    for _ in range(max_steps):
        act = np.nonzero(status >= MARCH)[0]
        if len(act) == 0:
            break
        in_flight.append(len(act))
        s_all = sdf_fn(o[act] + t[act, None] * d[act])
        for r, s in zip(act, s_all):
            steps[r] += 1
            if not np.isfinite(s):
                status[r] = NONFINITE
            elif abs(s) <= tol:
                status[r] = HIT
            elif status[r] == MARCH and s > 0:
                t_lo[r], s_lo[r] = t[r], s
                t[r] += max(omega * s, tol)
                if t[r] > far[r]:
                    status[r] = MISS
            elif status[r] == MARCH and steps[r] == 1:
                status[r] = START_INSIDE
            else:
                if status[r] == MARCH:
                    t_hi[r], s_hi[r], status[r] = t[r], s, REFINE
                elif s > 0:
                    if side[r] == 1:
                        s_hi[r] *= 0.5
                    t_lo[r], s_lo[r], side[r] = t[r], s, 1
                else:
                    if side[r] == 2:
                        s_lo[r] *= 0.5
                    t_hi[r], s_hi[r], side[r] = t[r], s, 2
                tn = t_lo[r] + (t_hi[r] - t_lo[r]) * (s_lo[r] / (s_lo[r] - s_hi[r]))
                if not t_lo[r] < tn < t_hi[r]:
                    tn = 0.5 * (t_lo[r] + t_hi[r])
                if not t_lo[r] < tn < t_hi[r]:      # adjacent numbers: nothing left to split
                    tn, status[r] = t_hi[r], HIT
                t[r] = tn
    status[status >= MARCH] = LIMIT
    return t, status, steps, in_flight


def segment_min(sdf_fn, o, d, a, b, n=SEGMENT_SAMPLES):
    """Smallest oracle sdf among n uniform samples of o + t d, t in [a, b], per ray (+inf where b < a)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(len(o), np.inf)
    ok = np.nonzero(b >= a)[0]
    if len(ok):
        ts = a[ok, None] + (b[ok] - a[ok])[:, None] * np.linspace(0.0, 1.0, n)[None, :]
        pts = o[ok, None, :] + ts[..., None] * d[ok, None, :]
        out[ok] = sdf_fn(pts.reshape(-1, 3)).reshape(len(ok), n).min(-1)
    return out


def light_block(direction, ambient=0.33, diffuse=0.66, specular=0.35, shininess=6.0):
    """The 16 floats of one light (oi_amd.relight.Light.packed)."""
    return [*direction, 0.0, *(ambient,) * 3, 0.0, *(diffuse,) * 3, 0.0, *(specular,) * 3, shininess]


def light_object_dir(direction, w2b):
    """The light's unit direction in the object frame: normalize(w2b[:3,:3] d / |d|)."""
    dd = np.asarray(direction, dtype=np.float64)
    l = np.asarray(w2b, dtype=np.float64)[:3, :3] @ (dd / np.linalg.norm(dd))
    return l / max(np.linalg.norm(l), 1e-6)


def shadow_rays(points, grad, l, bias=BIAS):
    """oi_trace_shadow_begin for one light: -> origins (n, 3), far (n,), traced (n,) bool (n . l > 0)."""
    n = A.unit(np.asarray(grad, dtype=np.float64))
    o = np.asarray(points, dtype=np.float64) + bias * n
    b, c = o @ l, (o * o).sum(-1) - 1.0
    disc = b * b - c
    far = np.where(disc > 0, np.maximum(np.sqrt(np.maximum(disc, 0.0)) - b, 0.0), 0.0)
    return o, far, (n @ l) > 0


def assert_secondary_begin_state(arr):
    """What oi_trace_shadow_begin and the oi_occlusion_*_begin entries leave in a state (arr: its arrays as torch tensors), read
    before the first step: the first sample point of every compacted ray is its origin bit for bit (o, not o + 0 d, which
    would lose the sign of a zero), bracket and side of every ray are zero bits, and t == near == 0."""
    bits = lambda t_: t_.detach().cpu().contiguous().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t_.element_size()])
    n0 = int(arr["counts"][0].item())
    assert 0 <= n0 <= arr["status"].numel()
    active = arr["active"].reshape(2, -1)[0, :n0].cpu().numpy().astype(np.int64)
    assert active.size == 0 or (active.min() >= 0 and active.max() < arr["status"].numel())
    assert np.array_equal(bits(arr["points"].reshape(-1, 3)[:n0]), bits(arr["rays_o"].reshape(-1, 3))[active]), "points != rays_o[active]"
    assert not bits(arr["bracket"]).any(), "bracket"
    assert not bits(arr["side"]).any(), "side"
    assert bool((arr["t"] == 0).all()) and bool((arr["near_"] == 0).all()), "t, near"


def visibility_of(status):
    """1 for a shadow ray that ended MISS, 0 for every other state."""
    return (np.asarray(status) == MISS).astype(np.float64)


def shade(ro, rd, t, grad, rgb, w2b, lights, bg=None, visibility=None):
    """oi_surface_shade on hit rays only, float64: image (L, 3, n) = Phong of relight_ref at weight 1 with one sample at
    depth t; with a visibility (L, n) the ambient part is kept and the rest scaled."""
    f = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
    n = len(t)
    lt = f(lights).reshape(-1, 16)
    args = (torch.ones(n, 1, dtype=torch.float64), f(grad).view(n, 1, 3), f(rgb).view(n, 1, 3), f(t).view(n, 1), f(ro), f(rd),
            f(w2b)[None])
    full = relight_ref(*args, lt, None, 1)["image_no_bg"][:, 0]
    if visibility is None:
        return full.numpy()
    amb = lt.clone()
    amb[:, 8:15] = 0.0       # no diffuse, no specular: ambient x albedo
    amb_img = relight_ref(*args, amb, None, 1)["image_no_bg"][:, 0]
    return (amb_img + f(visibility)[:, None, :] * (full - amb_img)).numpy()


def rehearse_primary(seed, pose_name, R=R_VIEW):
    """The primary-ray rehearsal of one view on the oracle alone.  -> dict of the figures the caps are stated on."""
    fld = Field(seed)
    ro, rd, near, far, w2b = view_rays(pose_name, R)
    t, status, steps, in_flight = trace(fld.sdf, ro, rd, near, far)
    hit, miss = status == HIT, status == MISS
    before = segment_min(fld.sdf, ro[hit], rd[hit], near[hit], t[hit] - SEGMENT_BACKOFF)
    along = segment_min(fld.sdf, ro[miss], rd[miss], near[miss], far[miss])
    return {"seed": seed, "pose": pose_name, "N": len(t), "hit": int(hit.sum()), "miss": int(miss.sum()),
            "limit": int((status == LIMIT).sum()), "start_inside": int((status == START_INSIDE).sum()),
            "nonfinite": int((status == NONFINITE).sum()), "evals_per_ray": sum(in_flight) / len(t),
            "hits_with_earlier_negative": int((before < 0).sum()), "misses_with_negative": int((along < 0).sum()),
            "steps_median_hit": float(np.median(steps[hit])) if hit.any() else 0.0,
            "_state": (fld, ro, rd, near, far, w2b, t, status, steps)}


def rehearse_shadows(state, light_dirs=LIGHT_DIRS, bias=BIAS):
    """Shadow rays of a rehearsed view under each light.  -> per light: traced, start_inside, limit, occluded, lit."""
    fld, ro, rd, near, far, w2b, t, status, steps = state
    hit = status == HIT
    pts = ro[hit] + t[hit, None] * rd[hit]
    _, g, _ = fld.full(pts)
    out = []
    for dd in light_dirs:
        l = light_object_dir(dd, w2b)
        o, sfar, traced = shadow_rays(pts, g, l, bias)
        n = int(traced.sum())
        ld = np.broadcast_to(l, (n, 3))
        _, st, _, _ = trace(fld.sdf, o[traced], ld, np.zeros(n), sfar[traced])
        out.append({"light": dd, "traced": n, "start_inside": int((st == START_INSIDE).sum()), "limit": int((st == LIMIT).sum()),
                    "occluded": int((st == HIT).sum()), "lit": int((st == MISS).sum())})
    return out
