"""Glossy environment lighting on the MI355X (include/oi_envgloss.h; oi_amd.envlight.EnvMap; oi_amd.trace.capture_transfer's
glossy_samples; oi_amd.inference.env_walk).  The references: the fp64 restatement tests/helpers/envgloss_ref.py fed the kernels'
own float32 inputs, include/oi_envlight.h's shading where the new entry must reproduce it bit for bit, and the analytic two-
sphere scene of tests/test_gpu_envlight.py, whose reflection-lobe visibility is integrated in float64.

Bars (EPS = 2^-24, half a unit in the last place of a number in [1, 2)):

  oi_env_prefilter     per output value, PF_SIGMAS = 6 standard deviations of the result about the exact sum, the deviation from
                       tests/helpers/envgloss_ref.py's prefilter_rounding_sigma: first-order propagation of independent
                       rounding errors (half an ulp per operation, one ulp for sincospif, v_log_f32 and v_exp_f32, each uniform
                       within its bound) through the header's expressions and through every partial sum of its two stages -- a
                       term passes through at most 32 + 8 + 8 additions in stage 1 and, for the <= 32 chunks of these cases,
                       32 in stage 2.  The lobe K = exp2(s log2 x) carries the error of its exponent e = s log2 x: 0.8 e^2 of
                       variance, so only terms with |e| < 24 (K > 2^-24) matter.  The error of the output texel's own direction
                       is common to all its terms and enters through the signed sum of their derivatives.  Six deviations of a
                       sum of many bounded errors are exceeded with probability < 1e-8 per value.  Measured on an MI355X: the
                       largest error is 0.233 of this bar (33 x 65 -> 9 x 17, s = 1), so the bar sits 4.3 x above the measured
                       margin; a worst-case bound (every error at its limit, all of one sign: 120 M + 34 D in units of EPS,
                       D the sum of the terms' derivatives) sat 17 x above it.  Relative to M = sum (w / pi) |L| K, the
                       magnitude of the sum, the errors are at most 9.9e-8 (s = 1), 9.4e-7 (s = 10) and 2.5e-5 (s = 200).
  oi_occlusion_lobe_begin   directions 64 EPS: the axis r = 2 ((n . v) n) - v of float32 n and v (2 ulp each from the
                       normalisation) is within 40 EPS, the polar law expf(logf(u1) / (s + 1)) within 23 EPS at |log| <= 3.1
                       (S = 256, s = 1), and the frame is the one oi_occlusion_ambient_begin is held to 1e-6 for.  Status and
                       counts agree exactly wherever |n . d| exceeds that bar; the rays nearer the horizon are at most 2 %.
  oi_env_shade_glossy  |k_s V| (coordinate error x the map's largest adjacent-texel difference + 8 EPS max |g|), the coordinate
                       error in texels (Hp dtheta / pi + Wp dphi / (2 pi)), dtheta = min(C EPS / sin theta, sqrt(2 C EPS)) and
                       dphi = min(C EPS / sin theta, pi): acos and atan2 of a direction within C EPS.  C = 64 (the axis' 40, two
                       3 x 3 rotations, acosf / atan2f); the kernel's coordinates are read back through a ramp map and their
                       distance from the float64 acos / atan2 is recorded in units of C.  At a pole the azimuth is not
                       conditioned at all and this bar allows any column of the polar row; there a second check holds the
                       result to a map whose polar rows are constant in phi, within 4 EPS (the two products of the header).
  analytic scene       5 standard errors of the S = 256 estimator, 5 * 0.5 / sqrt(256) = 0.156, against visibilities of 0.019
                       and 0.316 that would both be about 1 without the occluder."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_envlight as V
import test_gpu_trace as G
from conftest import record_margin
from helpers import env_ref as E
from helpers import envgloss_ref as Q
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
EPS = 2.0 ** -24
PF_SIGMAS = 6.0
DIR_BAR = 64 * EPS
ORIGIN_BAR, FAR_BAR = 1e-6, 1e-5            # test_gpu_occlusion's bars for the origins and the exit of the unit sphere
COORD_C = 64.0
_p, _cuda, _bits, _lib = V._p, V._cuda, V._bits, V._lib


# ---------------------------------------------------------------------------------------------------------------------
# oi_env_prefilter
# ---------------------------------------------------------------------------------------------------------------------
def _prefilter(img, s, Hp, Wp):
    lib, L, st = _lib()
    n_env, _, He, We = img.shape
    rad = guarded_copy(_cuda(img), "radiance")
    nf = L.oi_env_prefilter_partial_floats(n_env, He, We, Hp, Wp)
    assert nf == n_env * -(-He * We // Q.CHUNK) * 3 * Hp * Wp
    partial, out = guarded_empty((nf,), what="partial"), guarded_empty((n_env, 3, Hp, Wp), what="glossy")
    assert L.oi_env_prefilter(_p(rad), n_env, He, We, float(s), Hp, Wp, _p(partial), _p(out), st) == 0
    return out


def _signed_radiance(rs, shape):
    return (rs.uniform(0.25, 4.0, shape) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)


def _check_prefilter(img, s, Hp, Wp, case):
    out = _prefilter(img, s, Hp, Wp)
    ref, mag, _ = Q.prefilter(img, s, Hp, Wp)
    err = np.abs(npd(out) - ref)
    bar = PF_SIGMAS * EPS * Q.prefilter_rounding_sigma(img, s, Hp, Wp)
    assert (mag > 0).all()
    share = float((err / bar).max())
    print(case, "error over sum (w / pi) |L| K:", float((err / mag).max()), "bar over it:", float((bar / mag).max()),
          "error over bar:", share)
    record_margin(case, "err_over_abs_sum", float((err / mag).max()))
    record_margin(case, "err_over_bar", share)
    assert (err <= bar).all()
    return out


# the ragged sizes straddle every edge: 2145 input pixels are one chunk and 97 more, 153 outputs are part of one tile
@pytest.mark.parametrize("s", [1, 10, 200])
@pytest.mark.parametrize("n_env,He,We,Hp,Wp", [(1, 5, 7, 3, 5), (2, 8, 16, 4, 8), (3, 33, 65, 9, 17)])
def test_env_prefilter(n_env, He, We, Hp, Wp, s):
    rs = np.random.RandomState(He * 1000 + We * 10 + n_env + s)
    img = _signed_radiance(rs, (n_env, 3, He, We))
    case = f"env_prefilter[{He}x{We}->{Hp}x{Wp},E={n_env},s={s}]"
    out = _check_prefilter(img, s, Hp, Wp, case)
    assert torch.equal(_bits(out), _bits(_prefilter(img, s, Hp, Wp)))               # two launches: the same bytes
    for e in range(n_env if n_env > 1 else 0):
        assert torch.equal(_bits(out[e]), _bits(_prefilter(img[e:e + 1], s, Hp, Wp)[0])), e   # element e does not depend on E
    from oi_amd import ops
    assert torch.equal(_bits(ops.env_prefilter(_cuda(img), s, (Hp, Wp))), _bits(out))


# one input pixel fewer and one more than a chunk of 2048, the chunk itself; one output fewer and one more than a tile of 256
@pytest.mark.parametrize("He,We,Hp,Wp", [(23, 89, 3, 5), (32, 64, 3, 5), (3, 683, 3, 5), (5, 7, 15, 17), (5, 7, 1, 257)])
def test_env_prefilter_at_the_chunk_and_tile_edges(He, We, Hp, Wp):
    assert He * We in (Q.CHUNK - 1, Q.CHUNK, Q.CHUNK + 1) or Hp * Wp in (Q.TILE - 1, Q.TILE + 1)
    rs = np.random.RandomState(He + We + Hp + Wp)
    img = _signed_radiance(rs, (1, 3, He, We))
    out = _check_prefilter(img, 10, Hp, Wp, f"env_prefilter_edge[{He}x{We}->{Hp}x{Wp}]")
    assert torch.equal(_bits(out), _bits(_prefilter(img, 10, Hp, Wp)))


def test_env_prefilter_furnace_on_the_device():
    """The constant map on the GPU: 2 / (s + 1) within the restatement's 5e-3 plus the kernel's bar, on the 4 x 8 grid of the
    CPU furnace; and EnvMap.from_equirect holds the same bytes."""
    from oi_amd.envlight import EnvMap
    img = np.ones((1, 3, 32, 64), dtype=np.float32)
    for s in (1, 10, 50, 200):
        out = npd(_prefilter(img, s, 4, 8))
        assert np.abs(out * (s + 1) / 2.0 - 1.0).max() < 5e-3 + 1e-4, s
    env = EnvMap.from_equirect(img[0], 10, size=(4, 8))
    assert torch.equal(_bits(env.map), _bits(_prefilter(img, 10, 4, 8)[0])) and env.shininess == 10.0
    assert np.abs(env.sh.coeffs[0] - 2 * np.sqrt(np.pi)).max() < 1e-5 and np.array_equal(env.rotation, np.eye(3))


# ---------------------------------------------------------------------------------------------------------------------
# oi_occlusion_lobe_begin
# ---------------------------------------------------------------------------------------------------------------------
_lobe_inputs = Q.lobe_test_inputs


@pytest.mark.parametrize("s", [1, 10, 200])
@pytest.mark.parametrize("S", [1, 3, 256])
@pytest.mark.parametrize("n_hit", [1, 65, 130])
def test_lobe_begin(n_hit, S, s):
    lib, L, st = _lib()
    seed, bias = 11 + s, T.BIAS
    pts, grad, pix, eyes = Q.lobe_case(n_hit, S, s)
    o, d, far, traced, nd = Q.lobe_rays(pts, grad, pix, eyes[pix], S, float(s), seed, bias)
    # the restatement alone: the frame's branch (the sign of the axis' z) is not in doubt, and few rays graze the horizon
    _, _, r = Q.reflect(grad, pts, eyes[pix])
    assert (np.abs(r[:, 2]) > 1e-4).all()
    near_horizon = np.abs(nd) <= DIR_BAR
    assert near_horizon.mean() <= 0.02
    hp, g_t = guarded_copy(_cuda(pts), "hit_points"), guarded_copy(_cuda(grad), "grad")
    ro, hi = guarded_copy(_cuda(eyes), "rays_o"), guarded_copy(_cuda(pix, torch.int32), "hit_index")
    Qn = S * n_hit
    arr, St = V._guarded_state(Qn, "lobe")
    assert L.oi_occlusion_lobe_begin(ctypes.byref(St), _p(ro), _p(hp), _p(g_t), _p(hi), n_hit, S, float(s), bias, seed, st) == 0
    kd, ko = npd(arr["rays_d"]).reshape(S, n_hit, 3), npd(arr["rays_o"]).reshape(S, n_hit, 3)
    e_d, e_o = float(np.abs(kd - d).max()), float(np.abs(ko - o).max())
    e_f = float(np.abs(npd(arr["far_"]).reshape(S, n_hit) - far).max())
    case = f"lobe_begin[n_hit={n_hit},S={S},s={s}]"
    print(case, "directions", e_d, "bar", DIR_BAR, "origins", e_o, "far", e_f, "near the horizon", float(near_horizon.mean()))
    record_margin(case, "direction_err_over_bar", e_d / DIR_BAR)
    assert e_d <= DIR_BAR and e_o <= ORIGIN_BAR and e_f <= FAR_BAR
    assert np.abs(np.linalg.norm(kd, axis=-1) - 1).max() <= DIR_BAR
    status = arr["status"].cpu().numpy().reshape(S, n_hit)
    assert set(np.unique(status)) <= {T.MARCH, T.BACKFACING}
    clear = ~near_horizon
    assert np.array_equal(status[clear] == T.MARCH, traced[clear])
    n0 = int(arr["counts"][0].item())
    assert n0 == int((status == T.MARCH).sum()) and abs(n0 - int(traced.sum())) <= int(near_horizon.sum())
    assert not arr["counts"][1:].any()
    active = arr["active"][0, :n0].cpu().numpy()
    assert sorted(active.tolist()) == np.nonzero(status.reshape(-1) == T.MARCH)[0].tolist()
    assert torch.equal(arr["points"][:n0], arr["rays_o"][torch.as_tensor(active).long().cuda()])     # o + 0 d
    for name in ("near_", "t", "bracket"):
        assert not arr[name].any(), name
    assert not arr["side"].any() and not arr["steps"].any()
    T.assert_secondary_begin_state(arr)
    # a second launch: the same bytes; and through the wrapper
    arr2, St2 = V._guarded_state(Qn, "lobe2")
    assert L.oi_occlusion_lobe_begin(ctypes.byref(St2), _p(ro), _p(hp), _p(g_t), _p(hi), n_hit, S, float(s), bias, seed, st) == 0
    for name in ("rays_o", "rays_d", "far_", "status"):
        assert torch.equal(_bits(arr[name]), _bits(arr2[name])), name
    from oi_amd import ops
    ws = ops.TraceState(Qn, ref=ro)
    ops.occlusion_lobe_begin(ws, ro, hp, g_t, hi, n_hit, S, s, bias, seed)
    assert torch.equal(_bits(ws.rays_d), _bits(arr["rays_d"])) and torch.equal(ws.status, arr["status"])
    assert int(ws.counts[0].item()) == n0


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene: the point on top of the lower sphere, the field evaluated by torch between the steps
# ---------------------------------------------------------------------------------------------------------------------
def test_analytic_lobe_visibility():
    lib, L, st = _lib()
    S, s, per, bias = 256, 10.0, 3, Q.ANALYTIC_BIAS
    betas = (0.0, 0.6)
    want = [Q.analytic_lobe_visibility(b, s, n1=1000, n2=1000) for b in betas]
    assert abs(want[0] - 0.019) < 2e-3 and abs(want[1] - 0.316) < 3e-3
    bar = 5 * 0.5 / np.sqrt(S)
    n_hit, n_primary = per * len(betas), 40
    pts = np.broadcast_to(np.array([0.0, 0.0, E.R0]), (n_hit, 3)).astype(np.float32)
    pix = np.array([3, 17, 38, 5, 22, 31])
    eyes = np.zeros((n_primary, 3), dtype=np.float32)
    for k, b in enumerate(betas):
        eyes[pix[k * per:(k + 1) * per]] = Q.analytic_eye(b)
    hp, g_t = guarded_copy(_cuda(pts), "hit_points"), guarded_copy(_cuda(pts * 1.7), "grad")
    ro, hi = guarded_copy(_cuda(eyes), "rays_o"), guarded_copy(_cuda(pix, torch.int32), "hit_index")
    arr, St = V._guarded_state(S * n_hit, "lobe")
    assert L.oi_occlusion_lobe_begin(ctypes.byref(St), _p(ro), _p(hp), _p(g_t), _p(hi), n_hit, S, s, bias, R.SEED, st) == 0
    T.assert_secondary_begin_state(arr)
    steps = V._anyhit_loop(arr, St, V._two_spheres, 256)
    status = arr["status"].cpu().numpy().reshape(S, n_hit)
    assert status.max() <= T.BACKFACING
    slot_np = np.full(n_primary, -1)
    slot_np[pix] = np.arange(n_hit)
    slot = guarded_copy(_cuda(slot_np, torch.int32), "hit_slot")
    vis = guarded_empty((1, n_primary), what="spec_vis")
    assert L.oi_occlusion_resolve(_p(arr["status"]), _p(slot), n_primary, n_hit, 1, S, _p(vis), st) == 0
    got = npd(vis)[0]
    assert (got[slot_np < 0] == 1.0).all()
    open_sky = (status != T.BACKFACING).mean(0)                                     # without the occluder: the horizon alone
    for k, b in enumerate(betas):
        v = got[pix[k * per:(k + 1) * per]]
        print("analytic lobe visibility: beta", b, "V_spec", v, "expected", want[k], "bar", bar, "steps", steps,
              "above the horizon", open_sky[k * per:(k + 1) * per])
        record_margin("envgloss_analytic", f"beta={b}_err_over_bar", float(np.abs(v - want[k]).max() / bar))
        assert (np.abs(v - want[k]) <= bar).all()
        assert (open_sky[k * per:(k + 1) * per] > 0.95).all() and (v < 1.0 - 2 * bar).all()   # unoccluded it would be about 1


# ---------------------------------------------------------------------------------------------------------------------
# oi_env_shade_glossy
# ---------------------------------------------------------------------------------------------------------------------
class _ShadeCase:
    """One view's inputs on guarded buffers, and the restatement's side of them."""

    def __init__(self, rs, N, n_hit, F, maps):
        self.N, self.n_hit, self.F = N, n_hit, F
        self.slot_np = V._slots(rs, N, n_hit)
        self.mask = self.slot_np >= 0
        self.status_np = np.where(self.mask, T.HIT, rs.choice([T.MISS, T.LIMIT, T.START_INSIDE, T.NONFINITE], size=N)).astype(np.uint8)
        self.tr = rs.uniform(-1, 1, (9, N)).astype(np.float32)
        self.env = rs.randn(F, 9, 3).astype(np.float32)
        self.rgb, self.bg = rs.rand(n_hit, 3).astype(np.float32), np.array([0.1, 0.2, 0.3], dtype=np.float32)
        self.pts, self.grad, _, _ = _lobe_inputs(rs, max(n_hit, 1), max(n_hit, 1))
        self.pts, self.grad = self.pts[:n_hit], self.grad[:n_hit]
        self.eyes = (A.unit(rs.randn(N, 3)) * rs.uniform(1.5, 3.0, (N, 1))).astype(np.float32)
        self.w2b = V._w2b(rs)
        self.vis = rs.rand(N).astype(np.float32)
        self.maps = maps
        self.index = [int(v) for v in rs.randint(0, len(maps), F)]
        self.rot = np.stack([E.random_rotation(rs) for _ in range(F)]).astype(np.float32)
        self.ks = np.array([0.35, -0.2, 0.5], dtype=np.float32)
        self.alb = np.zeros((N, 3))
        self.alb[self.mask] = self.rgb[self.slot_np[self.mask]]

    def aim(self, f, pixel, target):
        """Turn environment f so that the lookup direction of `pixel` (on the mask) is `target`.  Replaces all of rot[f]."""
        k = self.slot_np[pixel]
        rw = Q.lookup_directions(self.grad[k:k + 1], self.pts[k:k + 1], self.eyes[pixel:pixel + 1], self.w2b, np.eye(3)[None])[0, 0]
        rw, t = rw / np.linalg.norm(rw), np.asarray(target, dtype=np.float64) / np.linalg.norm(target)
        ax = np.cross(t, rw)                                                        # R t = r_w, so that R^T r_w = t
        if np.linalg.norm(ax) < 1e-9:
            ax = np.cross(t, [1.0, 0.3, 0.2])
        self.rot[f] = E.axis_rotation(ax, np.arctan2(np.linalg.norm(np.cross(t, rw)), t @ rw)).astype(np.float32)

    def upload(self):
        c = lambda x, what, dt=torch.float32: guarded_copy(_cuda(x, dt), what)
        self.d = dict(status=c(self.status_np, "status", torch.uint8), slot=c(self.slot_np, "hit_slot", torch.int32),
                      rgb=c(self.rgb, "rgb") if self.n_hit else None, tr=c(self.tr, "transfer"), bg=c(self.bg, "bg"),
                      pts=c(self.pts, "hit_points") if self.n_hit else None, grad=c(self.grad, "grad") if self.n_hit else None,
                      eyes=c(self.eyes, "rays_o"), w2b=c(self.w2b, "w2b"), vis=c(self.vis, "spec_vis"), maps=c(self.maps, "glossy"),
                      ks=c(self.ks, "k_s"))
        return self

    def run(self, envs=None, rot=None, index=None, ks=None, vis="own", want=("shading", "image", "specular")):
        lib, L, st = _lib()
        envs = self.env if envs is None else envs
        F = len(envs)
        P = lib.EnvShadeParams()
        P.N, P.n_hit, P.F = self.N, self.n_hit, F
        out = {k: guarded_empty((F, 3, self.N), what=k) for k in want}
        d = self.d
        keep = [guarded_copy(_cuda(envs), "envs"), guarded_copy(_cuda(self.rot if rot is None else rot), "rot"),
                d["ks"] if ks is None else guarded_copy(_cuda(ks), "k_s")]
        for k_, v_ in dict(status=d["status"], hit_slot=d["slot"], rgb=d["rgb"], transfer=d["tr"], envs=keep[0], bg=d["bg"],
                           shading=out.get("shading"), image=out.get("image")).items():
            setattr(P, k_, _p(v_))
        idx = self.index if index is None else index
        v = d["vis"] if isinstance(vis, str) else vis
        M, _, Hp, Wp = self.maps.shape
        assert L.oi_env_shade_glossy(ctypes.byref(P), _p(d["eyes"]), _p(d["pts"]), _p(d["grad"]), _p(d["w2b"]), _p(v), _p(d["maps"]),
                                     M, Hp, Wp, (ctypes.c_int * F)(*idx), _p(keep[1]), _p(keep[2]), _p(out.get("specular")), st) == 0
        return out

    def reference(self):
        return Q.shade_glossy(self.tr, self.env, self.mask, self.slot_np, self.alb, self.grad, self.pts, self.eyes, self.w2b,
                              self.vis, self.maps, self.index, self.rot, self.ks, self.bg)

    def direction(self, f, pixel):
        """The float64 lookup direction of environment f at `pixel` (on the mask), from the float32 inputs the kernel gets."""
        k = self.slot_np[pixel]
        return Q.lookup_directions(self.grad[k:k + 1], self.pts[k:k + 1], self.eyes[pixel:pixel + 1], self.w2b, self.rot[f:f + 1])[0, 0]

    def specular_bar(self):
        """(F, 3, N): the docstring's bar of the specular output for the current rotations and map indices."""
        delta = np.array([Q.adjacent_difference(self.maps[m]).max() for m in self.index])
        gmax = np.array([np.abs(self.maps[m]).max() for m in self.index])
        kv = np.abs(self.ks)[None, :, None] * self.vis[None, None, :]
        return kv * (self.coordinate_error()[:, None, :] * delta[:, None, None] + 8 * EPS * gmax[:, None, None])

    def coordinate_error(self):
        """(F, N) texels, on the mask: the header's bound for a direction within COORD_C EPS of the exact one."""
        _, Hp, Wp = self.maps.shape[1:]
        err = np.zeros((self.F, self.N))
        if self.n_hit:
            k = self.slot_np[self.mask]
            d = Q.lookup_directions(self.grad[k], self.pts[k], self.eyes[self.mask], self.w2b, self.rot)
            # (acos is conditioned by 1 - z^2, atan2 by x^2 + y^2: the two differ where rounding left d short of unit length)
            sin_t = np.sqrt(np.minimum(np.maximum(1.0 - np.clip(d[..., 2], -1, 1) ** 2, 0.0), d[..., 0] ** 2 + d[..., 1] ** 2))
            c = COORD_C * EPS
            with np.errstate(divide="ignore"):
                dth = np.minimum(c / sin_t, np.sqrt(2 * c))
                dph = np.minimum(c / sin_t, np.pi)
            err[:, self.mask] = Hp * dth / np.pi + Wp * dph / (2 * np.pi)
        return err


def _maps(rs, M, Hp, Wp):
    """Random maps; the last one has its first and last rows constant in phi, as a prefiltered map nearly has: there the
    clamped lookup at a pole does not depend on the ill-conditioned azimuth."""
    g = rs.randn(M, 3, Hp, Wp).astype(np.float32)
    g[-1, :, 0, :], g[-1, :, -1, :] = g[-1, :, 0, :1], g[-1, :, -1, :1]
    return g


POLE_BAR = float(np.sqrt(2 * COORD_C * EPS))      # acos of a z within COORD_C EPS of +-1
AIMS = [("north pole", (0, 0, 1)), ("south pole", (0, 0, -1)), ("seam, phi > 0", (1, 1e-4, 0.2)), ("seam, phi < 2 pi", (1, -1e-4, 0.2))]


def _check_aimed_launches(c, N, F):
    """One launch per target, so every target survives: environment j % F is turned so that one pixel's reflected vector goes
    to the north pole, the south pole, and just either side of the seam phi = 0 | 2 pi.  The float64 directions actually used
    are asserted to be there; every pixel of the launch is held to the specular bar, and a pole pixel also to the constant
    polar row of the last map, where the clamp makes the result well conditioned (two roundings)."""
    Hp, Wp = c.maps.shape[2:]
    on = np.nonzero(c.mask)[0]
    rot0, index0 = c.rot.copy(), list(c.index)
    seen = set()
    for j, (name, tgt) in enumerate(AIMS):
        f, pixel = j % F, int(on[j % len(on)])
        c.rot, c.index = rot0.copy(), list(index0)
        c.aim(f, pixel, tgt)
        pole = name.endswith("pole")
        if pole:
            c.index[f] = len(c.maps) - 1
        d = c.direction(f, pixel)
        u, v = Q.lookup_coords(d, Hp, Wp)
        theta = float(np.arccos(np.clip(d[2], -1, 1)))
        if name == "north pole":
            assert theta <= POLE_BAR and np.floor(u) == -1                        # row -1, clamped to row 0
        elif name == "south pole":
            assert np.pi - theta <= POLE_BAR and np.floor(u) == Hp - 1            # row Hp, clamped to row Hp - 1
        elif name == "seam, phi > 0":
            assert 0 < np.arctan2(d[1], d[0]) < 1e-3 and np.floor(v) == -1        # columns Wp - 1 and 0
        else:
            assert -1e-3 < np.arctan2(d[1], d[0]) < 0 and np.floor(v) == Wp - 1   # columns Wp - 1 and 0, from the other side
        seen.add(name)
        got = npd(c.run(want=("specular",))["specular"])
        _, _, spec, _, _ = c.reference()
        err, bar = np.abs(got - spec), c.specular_bar()
        assert (err[:, :, c.mask] <= bar[:, :, c.mask]).all(), name
        if pole:
            row = c.maps[-1][:, 0 if name == "north pole" else Hp - 1, 0].astype(np.float64)
            want = c.ks.astype(np.float64) * float(c.vis[pixel]) * row
            e = np.abs(got[f, :, pixel] - want)
            record_margin(f"env_shade_glossy_pole[N={N},F={F}]", "err_over_4eps", float((e / (4 * EPS * np.abs(want))).max()))
            assert (e <= 4 * EPS * np.abs(want)).all(), (name, e, want)
        else:                                                                      # between the last and the first column
            i0 = int(np.floor(u))
            fu, fv = u - i0, v - np.floor(v)
            g = c.maps[c.index[f]].astype(np.float64)
            top = (1 - fv) * g[:, i0, Wp - 1] + fv * g[:, i0, 0]
            bot = (1 - fv) * g[:, i0 + 1, Wp - 1] + fv * g[:, i0 + 1, 0]
            want = c.ks.astype(np.float64) * float(c.vis[pixel]) * ((1 - fu) * top + fu * bot)
            assert (np.abs(got[f, :, pixel] - want) <= bar[f, :, pixel]).all(), name
    assert seen == {name for name, _ in AIMS}
    c.rot, c.index = rot0, index0


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 130])
def test_env_shade_glossy(N, F):
    lib, L, st = _lib()
    for n_hit in sorted({0, max(1, N // 2), N}):
        rs = np.random.RandomState(N * 100 + F * 10 + n_hit)
        maps = _maps(rs, 2, 5, 9)
        c = _ShadeCase(rs, N, n_hit, F, maps)
        c.upload()
        out = c.run()                                                            # random rotations
        sh, img, spec, mag, look = c.reference()
        bar_spec = c.specular_bar()
        bar_sh = 16 * EPS * mag
        e_spec, e_sh = np.abs(npd(out["specular"]) - spec), np.abs(npd(out["shading"]) - sh)
        e_img = np.abs(npd(out["image"]) - img)
        if n_hit:
            record_margin(f"env_shade_glossy[N={N},F={F}]", "specular_err_over_bar", float((e_spec / bar_spec)[:, :, c.mask].max()))
        assert (e_spec[:, :, c.mask] <= bar_spec[:, :, c.mask]).all() and (e_sh <= bar_sh).all()
        assert (e_img[:, :, c.mask] <= (bar_spec + bar_sh + 2 * EPS * np.abs(img))[:, :, c.mask]).all()
        # off the mask: no shading, no specular, the background
        off = ~c.mask
        assert not npd(out["shading"])[:, :, off].any() and not npd(out["specular"])[:, :, off].any()
        assert np.array_equal(npd(out["image"])[:, :, off], np.broadcast_to(c.bg.astype(np.float64)[None, :, None], (F, 3, int(off.sum()))))
        # any output may be absent
        for k in ("shading", "image", "specular"):
            assert torch.equal(_bits(c.run(want=(k,))[k]), _bits(out[k])), k
        # result f of the F-environment launch is the 1-environment launch of environment f, bit for bit
        for f in range(F):
            one = c.run(envs=c.env[f:f + 1], rot=c.rot[f:f + 1], index=c.index[f:f + 1])
            for k in out:
                assert torch.equal(_bits(one[k][0]), _bits(out[k][f])), (k, f)
        # k_s = 0: image and shading are oi_env_shade's bytes, the specular is 0
        zero = c.run(ks=np.zeros(3, dtype=np.float32))
        plain = V._shade(lib, L, st, N, n_hit, F, c.d["status"], c.d["slot"], c.d["rgb"], c.d["tr"], guarded_copy(_cuda(c.env), "envs"),
                         c.d["bg"])
        assert torch.equal(_bits(zero["image"]), _bits(plain["image"])) and torch.equal(_bits(zero["shading"]), _bits(plain["shading"]))
        assert torch.equal(_bits(out["shading"]), _bits(plain["shading"])) and not npd(zero["specular"]).any()
        # spec_vis = NULL is a map of ones
        ones = guarded_copy(torch.ones(N).cuda(), "ones")
        a, b = c.run(vis=None), c.run(vis=ones)
        for k in out:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        # both poles and both sides of the phi seam, a launch each
        if n_hit:
            _check_aimed_launches(c, N, F)
        # through the wrapper
        from oi_amd import ops
        via = ops.env_shade_glossy(c.d["status"], c.d["slot"], c.d["rgb"], n_hit, c.d["tr"], _cuda(c.env), c.d["eyes"], c.d["pts"],
                                   c.d["grad"], c.d["w2b"], c.d["vis"], c.d["maps"], c.index, _cuda(c.rot), c.d["ks"], c.d["bg"])
        for k in out:
            assert torch.equal(_bits(via[k]), _bits(out[k])), k


def test_lookup_coordinates_through_a_ramp_map():
    """A map whose first channel is the row number and whose second is the column number returns the kernel's own texel
    coordinates (inside the clamp and away from the wrap): their distance from the float64 acos / atan2 of the same inputs, in
    units of the bound that COORD_C stands for, is recorded and must not exceed 1."""
    rs = np.random.RandomState(9)
    Hp, Wp, N = 7, 12, 257
    ramp = np.zeros((1, 3, Hp, Wp), dtype=np.float32)
    ramp[0, 0] = np.arange(Hp)[:, None]
    ramp[0, 1] = np.arange(Wp)[None, :]
    c = _ShadeCase(rs, N, N, 2, ramp)
    c.index, c.ks, c.vis = [0, 0], np.ones(3, dtype=np.float32), np.ones(N, dtype=np.float32)
    out = npd(c.upload().run(want=("specular",))["specular"])
    k = c.slot_np
    d = Q.lookup_directions(c.grad[k], c.pts[k], c.eyes, c.w2b, c.rot)
    u, v = Q.lookup_coords(d, Hp, Wp)
    inside = (u > 0.01) & (u < Hp - 1.01) & (v > 0.01) & (v < Wp - 1.01)
    assert inside.mean() > 0.5
    bound = c.coordinate_error()
    share_u = float((np.abs(out[:, 0] - u) / bound)[inside].max())
    share_v = float((np.abs(out[:, 1] - v) / bound)[inside].max())
    print("lookup coordinates: error over the bound of C =", COORD_C, ": rows", share_u, "columns", share_v)
    record_margin("env_shade_glossy_coordinates", "err_over_bound", max(share_u, share_v))
    assert share_u <= 1.0 and share_v <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the golden field
# ---------------------------------------------------------------------------------------------------------------------
KS = (0.3, 0.2, 0.1)


def _tensors_equal(a, b, keys):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_constant_environment_end_to_end(precision, monkeypatch):
    from oi_amd import ops, trace
    from oi_amd.envlight import EnvLight, EnvMap
    from oi_amd.relight import Light
    gen, z, b2w = V._view(precision)
    s, H = 10.0, R.R_SOFT
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples=4, seed=R.SEED, glossy_samples=16, shininess=s)
    assert cap.spec_visibility.shape == (1, 1, H, H) and cap.shininess == s and cap.surface.glossy_state.N == 16 * cap.surface.n_hit
    st = cap.stats()
    assert st["glossy_evals"] > 0 and st["transfer_evals"] > 0
    out = cap.shade([EnvMap.constant(1.0, s)], bg=V.BG, specular=KS)
    assert set(out) == {"image", "shading", "specular"} and out["specular"].shape == (1, 3, H, H)
    mask = cap.maps["mask"][0, 0] > 0
    vis = cap.spec_visibility[0, 0]
    assert int(mask.sum()) > 50 and 0.0 < float(vis[mask].mean()) < 1.0 and bool((vis[~mask] == 1.0).all())
    want = torch.tensor(KS).cuda()[:, None, None] * vis[None] * (2.0 / (s + 1.0))
    err = float(((out["specular"][0] - want).abs() / want.abs().clamp(min=1e-30))[:, mask].max())
    print(f"envgloss_constant[{precision}] specular against k_s V_spec 2 / (s + 1): relative", err, "mean V_spec", float(vis[mask].mean()))
    record_margin(f"envgloss_constant[{precision}]", "specular_rel", err)
    assert err <= 4 * EPS and not bool(out["specular"][:, :, ~mask].any())
    # the diffuse half is the EnvLight path's, and the image is its image plus the specular
    plain = cap.shade([EnvLight.constant(1.0)], bg=V.BG)
    assert torch.equal(_bits(plain["shading"]), _bits(out["shading"]))
    assert float((out["image"] - (plain["image"] + out["specular"])).abs().max()) <= 4 * EPS * float(out["image"].abs().max())
    assert torch.equal(out["image"][0][:, ~mask], plain["image"][0][:, ~mask])
    # specular=None takes the generator's learned colour; a scalar is a grey one
    learned = Light.from_module(gen.light)
    assert cap.specular == learned.specular
    dflt, grey = cap.shade([EnvMap.constant(1.0, s)]), cap.shade([EnvMap.constant(1.0, s)], specular=0.3)
    assert torch.equal(_bits(dflt["specular"]), _bits(cap.shade([EnvMap.constant(1.0, s)], specular=learned.specular)["specular"]))
    assert torch.equal(_bits(grey["specular"][0, 0]), _bits(out["specular"][0, 0]))
    # shininess=None: the learned value
    assert trace._check_glossy(gen, 4, None, "x")[1] == learned.shininess
    # a capture without the new keywords, and one with glossy_samples = 0, launch what capture_transfer launched before

    def refuse(*a, **k):
        raise AssertionError("a reflection-lobe trace ran without glossy samples")
    monkeypatch.setattr(ops, "occlusion_lobe_begin", refuse)
    old = trace.capture_transfer(gen, z, b2w, transfer_samples=4, seed=R.SEED)
    zero = trace.capture_transfer(gen, z, b2w, transfer_samples=4, seed=R.SEED, glossy_samples=0, shininess=s)
    monkeypatch.undo()
    assert old.stats() == zero.stats() and old.stats()["glossy_evals"] == 0 and zero.spec_visibility is None
    assert torch.equal(_bits(old.transfer), _bits(zero.transfer)) and torch.equal(_bits(old.transfer), _bits(cap.transfer))
    st.pop("glossy_evals")
    assert {k: v for k, v in old.stats().items() if k in st} == st
    with pytest.raises(ValueError, match="no reflection-lobe trace"):
        old.shade([EnvMap.constant(1.0, s)])
    with pytest.raises(ValueError, match="shininess"):
        cap.shade([EnvMap.constant(1.0, 20.0)])
    flat = zero.shade([EnvMap.constant(1.0, s)], specular=KS)["specular"][0]          # V_spec = 1
    assert float((flat - torch.tensor(KS).cuda()[:, None, None] * (2.0 / (s + 1.0)) * mask).abs().max()) <= 4 * EPS


@pytest.mark.parametrize("precision", PRECISIONS)
def test_env_walk_over_a_map(precision, monkeypatch):
    """A walk over an EnvMap is one capture shaded under rotations of one prefiltered map, whatever the split into launches;
    nothing is prefiltered per frame."""
    from oi_amd import inference, ops, trace
    from oi_amd.envlight import EnvMap
    gen, z, b2w = V._view(precision)
    rs = np.random.RandomState(2)
    img = (rs.rand(3, 16, 32) * 2.0).astype(np.float32)
    img[:, 4:7, 5:9] += 20.0                                                        # a bright window: the walk is not symmetric
    env = EnvMap.from_equirect(img, 10.0, size=(8, 16))
    kw = dict(n_frames=5, axis=(0.2, -0.1, 1.0), transfer_samples=4, seed=R.SEED, bg=V.BG, glossy_samples=4, shininess=10.0,
              specular=KS)

    def refuse(*a, **k):
        raise AssertionError("the walk prefiltered a map")
    monkeypatch.setattr(ops, "env_prefilter", refuse)
    walk = inference.env_walk(gen, z, b2w, env, **kw)
    H = R.R_SOFT
    assert walk["image"].shape == walk["shading"].shape == walk["specular"].shape == (5, 3, H, H)
    assert walk["spec_visibility"].shape == (1, 1, H, H) and walk["stats"]["glossy_evals"] > 0
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples=4, seed=R.SEED, glossy_samples=4, shininess=10.0)
    assert torch.equal(cap.spec_visibility, walk["spec_visibility"])
    for i, Rm in enumerate(inference.env_walk_rotations(5, kw["axis"])):
        one = cap.shade([env.rotated(Rm)], bg=V.BG, specular=KS)
        for k in ("image", "shading", "specular"):
            assert torch.equal(_bits(one[k][0]), _bits(walk[k][i])), (k, i)
    assert not torch.equal(walk["specular"][0], walk["specular"][2])
    # the specular is k_s V_spec times the host lookup of the map along the G-buffer's reflected vector, frame by frame
    mask = npd(cap.maps["mask"]).reshape(-1) > 0
    s = cap.surface
    k = s.res.hit_slot.cpu().numpy()[mask]
    d0 = Q.lookup_directions(npd(s.grad)[k], npd(s.res.hit_points)[k], npd(s.ro)[mask], npd(s.w2b), np.eye(3)[None])[0]
    for i, Rm in enumerate(inference.env_walk_rotations(5, kw["axis"])):
        want = np.array(KS)[:, None] * npd(cap.spec_visibility).reshape(-1)[mask][None] * env.rotated(Rm).glossy(d0).T
        err = float(np.abs(npd(walk["specular"][i]).reshape(3, -1)[:, mask] - want).max())
        record_margin(f"envgloss_walk[{precision}]", "specular_vs_host_lookup", err)
        assert err <= 1e-4 * float(np.abs(npd(env.map)).max()), (i, err)
    launches = []
    shade = ops.env_shade_glossy

    def counting(*a, **k_):
        launches.append((a[5].shape[0], a[11].shape[0]))
        return shade(*a, **k_)
    monkeypatch.setattr(ops, "env_shade_glossy", counting)
    monkeypatch.setattr(trace, "ENV_MAX_ENVS", 2)
    split = inference.env_walk(gen, z, b2w, env, **kw)
    assert launches == [(2, 1), (2, 1), (1, 1)]                                     # rotations of one map share one index
    _tensors_equal(split, walk, ("image", "shading", "specular", "transfer", "mask", "spec_visibility"))
    # render_surface_env passes the keywords through
    monkeypatch.undo()
    one = trace.render_surface_env(gen, z, b2w, [env], transfer_samples=4, seed=R.SEED, bg=V.BG, glossy_samples=4, shininess=10.0,
                                   specular=KS)
    _tensors_equal({k: one[k][0] for k in ("image", "shading", "specular")}, {k: walk[k][0] for k in ("image", "shading", "specular")},
                   ("image", "shading", "specular"))
    assert one["glossy_trace"].N == 4 * cap.surface.n_hit and torch.equal(one["spec_visibility"], cap.spec_visibility)
