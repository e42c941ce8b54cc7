"""One diffuse interreflection bounce under environment lighting on the MI355X (include/oi_envbounce.h; oi_amd.trace.
capture_transfer(bounces=1) / render_surface_env; oi_amd.inference.env_walk).  The references: the fp64 restatement
tests/helpers/bounce_ref.py fed the kernels' own float32 inputs, oi_env_shade on the same inputs (a zero bounce changes
nothing), the furnace (a white object under a constant environment is shaded 1), and the analytic two-sphere scene of
tests/helpers/env_ref.py, whose bounce transfer is integrated in float64.

Bars (eps = 2^-24), derived from the kernels' operation sequences and never read off their output:
  oi_bounce_resolve    per output B[ch][c]: (K_band(c) + S + 2) eps M, M = the mean over the pixel's S samples of
                       [front-facing hit] rho_ch A_band(c) |y_c|max.  K counts the roundings behind one term A y_c(n_w) in units of
                       A |y_c|max: normalise (3 products, 2 additions, a square root, a division: 7) and rotate (3 products, 2
                       additions: 5) leave every component of n_w within 12 roundings; band 0 is a constant (K = 1); band 1
                       passes the 12 through and multiplies by k1 and by 2/3 (K = 14); band 2 is a quadratic form whose gradient
                       over its maximum is at most 3, plus at most 4 operations of its own, 1/4 being exact (K = 40).  Then one
                       fmaf multiplies by rho and adds (1), the S additions each round a partial sum of at most S M (S after the
                       division), and the division rounds once (1).  The front-face test n . d < 0 is a sign: the inputs keep
                       |n . d| >= 1e-3 (or exactly 0, a vanishing gradient), far above the 4 eps its float32 evaluation can be off
  oi_env_shade_bounce  19 eps sum_c (|T_c| + |B_c|) |L_c| for shading and indirect: 18 fmafs, each rounding a partial sum bounded
                       by that magnitude, and one addition; 20 for the image (one product more)
  furnace              (S + 16) eps about 1, the issue's: S accumulated terms, 16 for the constants and the two chains
  analytic scene       5 standard errors of the S = 256 estimator from the per-sample bound 0.5 rho A_band |y_c|max, i.e.
                       0.156 rho A |y|max, against T1_0 / rho = 0.153 (y_0 times the blocked share 0.54) and T1_2 / rho = -0.168;
                       T1[ch] / rho_ch agrees across channels within 2 (S + 1) eps A |y_c|max (each is S fmafs and a division
                       from the same sum); secondary hits lie on the blocker within tol + 8 eps (the float32 evaluation of the
                       field at the hit: 3 differences, 3 squares, 2 additions, a square root, a difference)
  golden view          oi_bounce_resolve's bar on the capture's own states.  The golden object is nearly convex (DESIGN section
                       4.18 measured an escaped share of 1.0), so few or none of its secondary rays end on it: that test pins
                       layout and plumbing, NOT interreflection, and does not assert that the share of rays that ended HIT is
                       positive; it prints and records it.  The analytic scene pins the physics.
  a view that sees     the golden field of latent 5 is not convex (47 of the 1952 transfer rays of its view "off" end on it, in
  itself               both precisions): the same bar there, where the second full MLP pass really runs"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_envlight as GE
import test_gpu_trace as G
from conftest import record_margin
from helpers import bounce_ref as B
from helpers import env_ref as E
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
EPS = B.EPS
OTHER_CODES = [T.MISS, T.LIMIT, T.START_INSIDE, T.NONFINITE, T.BACKFACING, T.MARCH, T.REFINE]
ND_MARGIN = 1e-3

_p, _cuda, _bits, _lib = GE._p, GE._cuda, GE._bits, GE._lib


# ---------------------------------------------------------------------------------------------------------------------
# oi_bounce_resolve
# ---------------------------------------------------------------------------------------------------------------------
def _resolve_case(rs, N, S, kind, white=False, codes=OTHER_CODES):
    """Three pixels off the mask (as many as N - 1 allows), a permuted hit_slot, every final state present where the rays
    allow it, n_hit2 = 0 / 1 / half the rays, front and back faces, one vanishing gradient; |n . d| >= ND_MARGIN or 0."""
    n_hit = N - min(3, N - 1)
    Q = S * n_hit
    status = rs.choice(codes, size=Q).astype(np.uint8)
    perm = rs.permutation(Q)
    reserve = len(codes) if Q >= 16 else 0
    status[perm[:reserve]] = codes[:reserve]
    n2 = {"none": 0, "one": 1, "half": max(1, Q // 2)}[kind]
    hits = perm[reserve:reserve + n2]
    status[hits] = T.HIT
    slot2 = np.full(Q, -1)
    slot2[hits] = rs.permutation(n2)
    grad2 = (A.unit(rs.randn(n2, 3)) * rs.uniform(0.3, 3.0, (n2, 1))).astype(np.float32)
    if n2 >= 3 and not white:
        grad2[1] = 0.0                                                       # below the 1e-6 of the normalisation: n = 0
    d = A.unit(rs.randn(Q, 3)).astype(np.float32)
    nrm = A.unit(grad2.astype(np.float64)) if n2 else np.zeros((0, 3))
    for _ in range(64):                                                      # keep the sign of n . d out of doubt
        nd = (nrm[slot2[hits]] * d[hits].astype(np.float64)).sum(-1)
        near = (np.abs(nd) < ND_MARGIN) & (np.linalg.norm(grad2[slot2[hits]], axis=-1) > 0)
        if not near.any():
            break
        d[hits[near]] = A.unit(rs.randn(int(near.sum()), 3)).astype(np.float32)
    assert not near.any()
    if white:                                                                # the furnace: every hit a front face
        flip = (nrm[slot2[hits]] * d[hits]).sum(-1) >= 0
        d[hits[flip]] *= -1.0
    rgb2 = np.ones((n2, 3), dtype=np.float32) if white else rs.rand(n2, 3).astype(np.float32)
    return n_hit, status, d, slot2, grad2, rgb2, GE._slots(rs, N, n_hit), GE._w2b(rs)


def _upload(status, d, slot2, grad2, rgb2, slot_np, w2b_np, n_hit):
    g = lambda a, dt, what: guarded_copy(_cuda(a, dt), what) if len(a) else None
    return (g(status, torch.uint8, "status") if n_hit else None, g(d, torch.float32, "rays_d") if n_hit else None,
            g(slot2, torch.int32, "hit_slot2") if n_hit else None, g(grad2, torch.float32, "grad2"), g(rgb2, torch.float32, "rgb2"),
            guarded_copy(_cuda(slot_np, torch.int32), "hit_slot"), guarded_copy(_cuda(w2b_np), "w2b"))


def _bounce(L, st, dev, N, n_hit, n2, S):
    status, d, slot2, grad2, rgb2, slot, w2b = dev
    out = guarded_empty((3, 9, N), what="bounce")
    assert L.oi_bounce_resolve(_p(status), _p(d), _p(slot2), _p(grad2), _p(rgb2), _p(slot), N, n_hit, n2, S, _p(w2b), _p(out), st) == 0
    return out


@pytest.mark.parametrize("N,S", [(1, 1), (1, 3), (63, 1), (63, 3), (65, 1), (65, 3), (65, 256), (257, 1), (257, 3)])
def test_bounce_resolve(N, S):
    lib, L, st = _lib()
    worst = 0.0
    for kind in ("none", "one", "half"):
        rs = np.random.RandomState(N * 1000 + S * 7 + len(kind))
        n_hit, status, d, slot2, grad2, rgb2, slot_np, w2b_np = _resolve_case(rs, N, S, kind)
        n2 = len(grad2)
        if S * n_hit >= 16:
            assert set(status.tolist()) >= set(OTHER_CODES) and ((status == T.HIT).sum() == n2)
        dev = _upload(status, d, slot2, grad2, rgb2, slot_np, w2b_np, n_hit)
        assert (dev[3] is None) == (n2 == 0)                                  # n_hit2 = 0 runs with NULL grad2 / rgb2
        outs = [_bounce(L, st, dev, N, n_hit, n2, S) for _ in range(2)]
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
        ref, mag, nd, front = B.resolve(status, d, slot2, grad2 if n2 else None, rgb2 if n2 else None, slot_np, n_hit, S, w2b_np)
        got = npd(outs[0])
        bar = B.resolve_bar(mag, S)
        err = np.abs(got - ref)
        assert (err <= bar).all(), (kind, float((err - bar).max()))
        if (bar > 0).any():
            worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()))
        assert not got[:, :, slot_np < 0].any()                               # exact zeros off the mask
        if kind == "none":
            assert not got.any()
        if kind == "half" and S * n_hit >= 64:
            hit = (status == T.HIT).reshape(S, n_hit)
            assert front.any() and (hit & ~front).any() and np.abs(ref).max() > 0.01      # front and back faces both occur
        from oi_amd import ops
        if n_hit:
            via = ops.bounce_resolve(dev[0], dev[1], dev[2], dev[3], dev[4], n2, dev[5], N, n_hit, S, dev[6])
            assert torch.equal(_bits(via), _bits(outs[0]))
    print(f"bounce_resolve[N={N},S={S}] worst error over the bar", worst)
    record_margin(f"bounce_resolve[N={N},S={S}]", "err_over_bar", worst)


# ---------------------------------------------------------------------------------------------------------------------
# oi_env_shade_bounce
# ---------------------------------------------------------------------------------------------------------------------
def _shade(L, st, N, n_hit, F, status, slot, rgb, transfer, bounce, envs, bg, want=("shading", "image", "indirect")):
    from oi_amd import lib
    P = lib.EnvShadeBounceParams()
    P.N, P.n_hit, P.F = N, n_hit, F
    out = {k: guarded_empty((F, 3, N), what=k) for k in want}
    for k_, v_ in dict(status=status, hit_slot=slot, rgb=rgb, transfer=transfer, envs=envs, bg=bg, bounce=bounce,
                       shading=out.get("shading"), image=out.get("image"), indirect=out.get("indirect")).items():
        setattr(P, k_, _p(v_))
    assert L.oi_env_shade_bounce(ctypes.byref(P), st) == 0
    return out


@pytest.mark.parametrize("N,F", [(1, 1), (1, 3), (65, 1), (65, 3), (65, 256), (257, 1), (257, 3)])
def test_env_shade_bounce(N, F):
    lib, L, st = _lib()
    from oi_amd import ops
    for n_hit in sorted({0, max(1, N - 1)}):
        rs = np.random.RandomState(N * 1000 + F + n_hit)
        slot_np = GE._slots(rs, N, n_hit)
        mask = slot_np >= 0
        status_np = np.where(mask, T.HIT, rs.choice([T.MISS, T.LIMIT, T.START_INSIDE, T.NONFINITE], size=N)).astype(np.uint8)
        tr_np = rs.uniform(-1, 1, (9, N)).astype(np.float32)                  # non-zero off the mask too: the kernel masks
        bo_np = rs.uniform(-0.5, 0.5, (3, 9, N)).astype(np.float32)
        env_np = rs.randn(F, 9, 3).astype(np.float32)
        if n_hit:
            env_np[0, :, 0] = -(tr_np + bo_np[0])[:, np.nonzero(mask)[0][0]]   # a pixel whose shading is -|T + B|^2 < 0
        rgb_np, bg_np = rs.rand(n_hit, 3).astype(np.float32), np.array([0.1, 0.2, 0.3], dtype=np.float32)
        status, slot = guarded_copy(_cuda(status_np, torch.uint8), "status"), guarded_copy(_cuda(slot_np, torch.int32), "hit_slot")
        rgb = guarded_copy(_cuda(rgb_np), "rgb") if n_hit else None
        transfer, bounce = guarded_copy(_cuda(tr_np), "transfer"), guarded_copy(_cuda(bo_np), "bounce")
        envs, bg = guarded_copy(_cuda(env_np), "envs"), guarded_copy(_cuda(bg_np), "bg")
        out = _shade(L, st, N, n_hit, F, status, slot, rgb, transfer, bounce, envs, bg)
        alb = np.zeros((N, 3))
        alb[mask] = rgb_np[slot_np[mask]]
        sh, ind, img, mag = B.shade(tr_np, bo_np, env_np, mask, alb, bg_np)
        bar = B.SHADE_ROUNDINGS * EPS * mag
        e_sh, e_in = np.abs(npd(out["shading"]) - sh), np.abs(npd(out["indirect"]) - ind)
        e_img = np.abs(npd(out["image"]) - img)
        if n_hit:
            record_margin(f"env_shade_bounce[N={N},F={F}]", "err_over_bar", float((np.maximum(e_sh, e_in) / bar)[:, :, mask].max()))
        assert (e_sh <= bar).all() and (e_in <= bar).all() and (e_img <= (B.SHADE_ROUNDINGS + 1) * EPS * mag).all()
        # off the mask: shading and indirect 0, image the background, exactly
        assert not npd(out["shading"])[:, :, ~mask].any() and not npd(out["indirect"])[:, :, ~mask].any()
        assert np.array_equal(npd(out["image"])[:, :, ~mask],
                              np.broadcast_to(bg_np.astype(np.float64)[None, :, None], (F, 3, int((~mask).sum()))))
        if n_hit:
            neg = npd(out["shading"])[:, :, mask] < 0
            assert neg.any() and not npd(out["image"])[:, :, mask][neg].any()  # clamped in the image, kept in the shading
        black = _shade(L, st, N, n_hit, F, status, slot, rgb, transfer, bounce, envs, None, want=("image",))
        assert not npd(black["image"])[:, :, ~mask].any()
        # each output may be absent
        for k in ("shading", "image", "indirect"):
            only = _shade(L, st, N, n_hit, F, status, slot, rgb, transfer, bounce, envs, bg, want=(k,))
            assert torch.equal(_bits(only[k]), _bits(out[k])), k
        # result f of the F-environment launch is the 1-environment launch of environment f, bit for bit
        for f in sorted({0, F // 3, F - 1}):
            one = _shade(L, st, N, n_hit, 1, status, slot, rgb, transfer, bounce, guarded_copy(_cuda(env_np[f:f + 1]), "env1"), bg)
            for k in ("shading", "image", "indirect"):
                assert torch.equal(_bits(one[k][0]), _bits(out[k][f])), (k, f)
        # a zero bounce: oi_env_shade's shading and image on the same inputs
        zero = guarded_copy(torch.zeros(3, 9, N).cuda(), "bounce0")
        z = _shade(L, st, N, n_hit, F, status, slot, rgb, transfer, zero, envs, bg)
        plain = GE._shade(lib, L, st, N, n_hit, F, status, slot, rgb, transfer, envs, bg)
        assert torch.equal(z["shading"], plain["shading"]) and torch.equal(z["image"], plain["image"])
        assert not bool(z["indirect"].any())
        via = ops.env_shade_bounce(status, slot, rgb, n_hit, transfer, bounce, envs, bg)
        for k in ("shading", "image", "indirect"):
            assert torch.equal(_bits(via[k]), _bits(out[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# the furnace through the three kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 256])
def test_furnace(S):
    """A white object under the constant environment: every pixel whose rays all end MISS or on a front face is shaded 1."""
    lib, L, st = _lib()
    from oi_amd.envlight import EnvLight, stack_envs
    N = 65
    rs = np.random.RandomState(S)
    n_hit, status, d, slot2, grad2, rgb2, slot_np, w2b_np = _resolve_case(rs, N, S, "half", white=True, codes=[T.MISS])
    q = []                                                                    # up to five pixels with a ray that bounces nothing
    for i in rs.permutation(n_hit)[:5]:
        js = np.nonzero(status.reshape(S, n_hit)[:, i] == T.MISS)[0]
        q += [js[0] * n_hit + i] if len(js) else []
    q = np.array(q)
    status[q] = T.LIMIT
    n2 = len(grad2)
    dev = _upload(status, d, slot2, grad2, rgb2, slot_np, w2b_np, n_hit)
    bounce = _bounce(L, st, dev, N, n_hit, n2, S)
    transfer = guarded_empty((9, N), what="transfer")
    assert L.oi_transfer_resolve(_p(dev[0]), _p(dev[1]), _p(dev[5]), N, n_hit, S, _p(dev[6]), _p(transfer), st) == 0
    _, _, _, front = B.resolve(status, d, slot2, grad2, rgb2, slot_np, n_hit, S, w2b_np)
    assert front.sum() == (status == T.HIT).sum() > 0
    ok = ((status == T.MISS).reshape(S, n_hit) | front).all(0)                # per hit slot
    assert ok.sum() >= n_hit - 5 and (~ok).sum() == len(set((q % n_hit).tolist())) > 0
    mask = slot_np >= 0
    prim = guarded_copy(_cuda(np.where(mask, T.HIT, T.MISS), torch.uint8), "status1")
    rgb = guarded_copy(torch.ones(n_hit, 3).cuda(), "rgb")
    envs = guarded_copy(stack_envs([EnvLight.constant(1)]), "envs")
    out = _shade(L, st, N, n_hit, 1, prim, dev[5], rgb, transfer, bounce, envs, None)
    sh = npd(out["shading"])[0]
    pix_ok = np.zeros(N, dtype=bool)
    pix_ok[mask] = ok[slot_np[mask]]
    err = float(np.abs(sh[:, pix_ok] - 1.0).max())
    bar = (S + 16) * EPS
    print(f"bounce_furnace[S={S}] |shading - 1|", err, "bar", bar, "indirect share", float(npd(out["indirect"])[0][:, pix_ok].mean()))
    record_margin(f"bounce_furnace[S={S}]", "err_over_bar", err / bar)
    assert err <= bar
    assert (sh[:, mask & ~pix_ok] < 1.0 - 0.5 / S).all()                      # a ray that bounces nothing is missing from the sum
    assert torch.equal(out["image"], out["shading"].clamp(min=0))             # albedo 1, no background


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene, through the C ABI on guarded buffers, the field evaluated by torch between the steps
# ---------------------------------------------------------------------------------------------------------------------
def _closest_loop(arr, S, field, max_steps):
    """oi_trace_step until no ray is in flight, then oi_trace_finish.  -> steps run, hit_index, hit_points, hit_slot, n_hit2."""
    lib, L, st = _lib()
    Q = S.N
    bound, k = int(arr["counts"][0].item()), 0
    while bound > 0 and k < max_steps:
        sdf = guarded_copy(field(arr["points"][:bound]), "sdf")
        assert L.oi_trace_step(ctypes.byref(S), _p(sdf), bound, k, T.TOL, T.OMEGA, st) == 0
        k += 1
        bound = int(arr["counts"][k].item())
    hit_index = guarded_empty((Q,), torch.int32, what="f_hit_index", must_write=False)
    hit_points = guarded_empty((Q, 3), what="f_hit_points", must_write=False)
    hit_slot = guarded_empty((Q,), torch.int32, what="f_hit_slot")
    assert L.oi_trace_finish(ctypes.byref(S), _p(hit_index), _p(hit_points), _p(hit_slot), st) == 0
    return k, hit_index, hit_points, hit_slot, int(arr["counts"][-1].item())


def test_analytic_bounce_under_the_blocker():
    """Three pixels at the point on top of the lower sphere, directly under the upper one, and one on the lower sphere's equator,
    which sees nothing.  The transfer rays are marched twice from the same begin: with the any-hit step and with the closest-
    hit step.  The direct transfer is the same bytes; the closest hits lie on the upper sphere; with its analytic normals and
    the albedo (0.9, 0.5, 0.1) the bounce transfer under the blocker is the quadrature's within 5 standard errors."""
    lib, L, st = _lib()
    S = 256
    rho = np.array([0.9, 0.5, 0.1], dtype=np.float32)
    pts = np.array([[0.0, 0.0, E.R0]] * 3 + [[E.R0, 0.0, 0.0]])
    nrm = pts / E.R0
    n_hit, pix = 4, np.array([11, 4, 300, 77])
    hp, grad = guarded_copy(_cuda(pts), "hit_points"), guarded_copy(_cuda(nrm * 1.7), "grad")
    hit_index = guarded_copy(_cuda(pix, torch.int32), "hit_index")
    states = []
    for tag in ("any", "closest"):
        arr, St = GE._guarded_state(S * n_hit, tag)
        assert L.oi_occlusion_ambient_begin(ctypes.byref(St), _p(hp), _p(grad), _p(hit_index), n_hit, S, T.BIAS, 4.0, R.SEED, st) == 0
        T.assert_secondary_begin_state(arr)
        states.append((arr, St))
    (arr_a, St_a), (arr_c, St_c) = states
    assert torch.equal(_bits(arr_a["rays_d"]), _bits(arr_c["rays_d"])) and torch.equal(_bits(arr_a["rays_o"]), _bits(arr_c["rays_o"]))
    steps_a = GE._anyhit_loop(arr_a, St_a, GE._two_spheres, 256)
    steps_c, _, hit_points2, hit_slot2, n2 = _closest_loop(arr_c, St_c, GE._two_spheres, 256)
    st_a, st_c = arr_a["status"].cpu().numpy(), arr_c["status"].cpu().numpy()
    assert st_c.max() <= T.NONFINITE and np.array_equal(st_a == T.MISS, st_c == T.MISS)
    assert (st_c.reshape(S, n_hit)[:, 3] == T.MISS).all()                     # the equator sees nothing
    slot_np = np.array([2, -1, 0, 1, 3])
    slot, w2b = guarded_copy(_cuda(slot_np, torch.int32), "hit_slot"), guarded_copy(torch.eye(4).cuda(), "w2b")
    direct = []
    for arr in (arr_a, arr_c):
        out = guarded_empty((9, 5), what="transfer")
        assert L.oi_transfer_resolve(_p(arr["status"]), _p(arr["rays_d"]), _p(slot), 5, n_hit, S, _p(w2b), _p(out), st) == 0
        direct.append(out)
    assert torch.equal(_bits(direct[0]), _bits(direct[1]))                    # T0 of the bounce trace is today's, bit for bit
    # the secondary hits: every HIT is listed, and lies on the blocker
    assert n2 == int((st_c == T.HIT).sum()) > 0.4 * 3 * S
    s2 = hit_slot2.cpu().numpy()
    assert np.array_equal(s2 >= 0, st_c == T.HIT) and sorted(s2[s2 >= 0].tolist()) == list(range(n2))
    hp2 = npd(hit_points2)[:n2]
    off = np.abs(np.linalg.norm(hp2 - E.C1, axis=-1) - E.R1)
    print("analytic bounce: steps any-hit", steps_a, "closest-hit", steps_c, "secondary hits", n2, "of", 3 * S,
          "worst distance from the blocker", float(off.max()))
    assert off.max() <= T.TOL + 8 * EPS
    c1 = torch.tensor(E.C1, dtype=torch.float32).cuda()
    grad2 = guarded_copy(((hit_points2[:n2] - c1) / E.R1 * 1.7).contiguous(), "grad2")
    rgb2 = guarded_copy(_cuda(np.tile(rho, (n2, 1))), "rgb2")
    outs = []
    for _ in range(2):
        out = guarded_empty((3, 9, 5), what="bounce")
        assert L.oi_bounce_resolve(_p(arr_c["status"]), _p(arr_c["rays_d"]), _p(hit_slot2), _p(grad2), _p(rgb2), _p(slot), 5, n_hit, n2,
                                   S, _p(w2b), _p(out), st) == 0
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    t1 = npd(outs[0])
    ref, mag, _, front = B.resolve(st_c, npd(arr_c["rays_d"]), s2, npd(grad2), npd(rgb2), slot_np, n_hit, S, np.eye(4))
    assert (np.abs(t1 - ref) <= B.resolve_bar(mag, S)).all() and front.sum() > 0.9 * n2
    assert not t1[:, :, 1].any() and not t1[:, :, 4].any()                    # off the mask; the equator: exactly 0
    quad = B.top_quadrature()
    under = t1[:, :, [2, 3, 0]]                                               # the pixels of slots 0, 1, 2
    worst = 0.0
    for ch in range(3):
        bar = B.standard_error_bar(S, float(rho[ch]))
        err = np.abs(under[ch] - float(rho[ch]) * quad[:, None])
        worst = max(worst, float((err / bar[:, None]).max()))
        assert (err <= bar[:, None]).all(), (ch, err.max(1), bar)
        ratio = np.abs(under[ch] / float(rho[ch]) - under[0] / float(rho[0]))
        assert (ratio <= 2 * (S + 1) * EPS * B.A_Y_MAX[:, None]).all(), (ch, ratio.max(1))
    print("analytic bounce: T1 / rho under the blocker", under[0][[0, 2, 6]].T / float(rho[0]), "quadrature", quad[[0, 2, 6]],
          "worst error over the 5-standard-error bar", worst)
    record_margin("envbounce_analytic", "T1_err_over_bar", worst)
    assert (under[0][0] > 0.1 * float(rho[0])).all() and (under[0][2] < 0).all()   # the blocker's underside faces down


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the golden field
# ---------------------------------------------------------------------------------------------------------------------
SEED, POSE = R.SOFT_VIEWS[0]
BG = (0.1, 0.2, 0.3)
TRACE_OPS = {"trace_begin", "trace_step", "trace_finish", "sdf_mlp_fwd", "occlusion_ambient_begin", "occlusion_step",
             "occlusion_lobe_begin", "occlusion_resolve", "transfer_resolve", "transfer_normal", "bounce_resolve", "surface_shade",
             "surface_shade_ao", "env_shade", "env_shade_bounce", "env_shade_glossy"}


def _view(precision):
    return G.make_gen(precision, R.R_SOFT), A.latent(SEED)[0], T.pose(POSE)


def _record_ops(monkeypatch):
    """Every public function of oi_amd.ops appends its name to the returned list when called; trace._march appends
    ('march', anyhit)."""
    import types
    from oi_amd import ops, trace
    calls = []

    def wrap(name, fn):
        def counted(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return counted
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
            monkeypatch.setattr(ops, name, wrap(name, fn))
    march = trace._march

    def counted_march(*a, anyhit=False, **k):
        calls.append(("march", anyhit))
        return march(*a, anyhit=anyhit, **k)
    monkeypatch.setattr(trace, "_march", counted_march)
    return calls


@pytest.mark.parametrize("precision", PRECISIONS)
def test_capture_with_a_bounce(precision, monkeypatch):
    """The golden view: the direct transfer of a bounce capture is the plain capture's bit for bit, the bounce map is the
    restatement's on the capture's own states, shade() returns the indirect part, a split walk is the unsplit one, and a
    bounces=0 capture launches what a call without the keyword launches.  The object is nearly convex: this pins layout and
    plumbing, not interreflection (test_analytic_bounce_under_the_blocker pins the physics), and the share of secondary rays
    that ended HIT is printed and recorded, never asserted positive."""
    from oi_amd import inference, ops, trace
    from oi_amd.envlight import EnvLight
    gen, z, b2w = _view(precision)
    S, H = 16, R.R_SOFT
    plain = trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED)
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED, bounces=1)
    assert plain.bounce is None and cap.bounce.shape == (1, 3, 9, H, H)
    assert torch.equal(_bits(cap.transfer), _bits(plain.transfer))
    s = cap.surface
    st, hits = s.transfer_state, s.bounce_hits
    n2 = hits["n_hit"]
    status = st.status.cpu().numpy()
    assert st.N == S * s.n_hit and int(status.max()) <= T.BACKFACING and n2 == int((status == T.HIT).sum())
    assert cap.stats()["bounce_points"] == n2 and plain.stats()["bounce_points"] == 0 and cap.stats()["transfer_evals"] > 0
    share = n2 / float(st.N)
    print(f"envbounce_capture[{precision}] secondary rays that ended HIT", n2, "of", st.N, "share", share,
          "escaped", float((status == T.MISS).mean()))
    record_margin(f"envbounce_capture[{precision}]", "hit_share", share)
    ref, mag, _, _ = B.resolve(status, npd(st.rays_d), hits["hit_slot"].cpu().numpy(), npd(hits["grad"]) if n2 else None,
                               npd(hits["rgb"]) if n2 else None, s.res.hit_slot.cpu().numpy(), s.n_hit, S, npd(s.w2b))
    got = npd(cap.bounce).reshape(3, 9, -1)
    bar = B.resolve_bar(mag, S)
    err = np.abs(got - ref)
    if (bar > 0).any():
        record_margin(f"envbounce_capture[{precision}]", "err_over_bar", float((err[bar > 0] / bar[bar > 0]).max()))
    assert (err <= bar).all()
    # shade: the indirect part is returned, and shading - indirect is the direct shade
    envs = [EnvLight(np.random.RandomState(2).randn(9, 3) * 0.5 + np.eye(9)[0][:, None] * 3.0), EnvLight.constant((1.0, 0.5, 0.25))]
    a, b = plain.shade(envs, bg=BG), cap.shade(envs, bg=BG)
    assert set(a) == {"shading", "image"} and set(b) == {"shading", "image", "indirect"} and b["indirect"].shape == (2, 3, H, H)
    D, I, Sh = npd(a["shading"]), npd(b["indirect"]), npd(b["shading"])
    assert (np.abs((Sh - I) - D) <= EPS * (np.abs(D) + np.abs(I))).all()
    mask = cap.maps["mask"][0, 0] > 0
    assert not bool(b["indirect"][:, :, ~mask].any()) and torch.equal(_bits(b["image"][:, :, ~mask]), _bits(a["image"][:, :, ~mask]))
    # render_surface_env and env_walk pass the keyword through
    out = trace.render_surface_env(gen, z, b2w, envs, transfer_samples=S, seed=R.SEED, bg=BG, bounces=1)
    for k in ("shading", "image", "indirect"):
        assert torch.equal(_bits(out[k]), _bits(b[k])), k
    assert torch.equal(_bits(out["bounce"]), _bits(cap.bounce)) and out["stats"]["bounce_points"] == n2
    kw = dict(n_frames=5, axis=(0.2, -0.1, 1.0), transfer_samples=S, seed=R.SEED, bg=BG, bounces=1)
    walk = inference.env_walk(gen, z, b2w, envs[0], **kw)
    assert walk["indirect"].shape == (5, 3, H, H) and torch.equal(_bits(walk["bounce"]), _bits(cap.bounce))
    for i, Rm in enumerate(inference.env_walk_rotations(5, kw["axis"])):
        one = cap.shade([envs[0].rotated(Rm)], bg=BG)
        for k in ("shading", "image", "indirect"):
            assert torch.equal(_bits(one[k][0]), _bits(walk[k][i])), (k, i)
    launches = []
    shade = ops.env_shade_bounce

    def counting(*a_, **k_):
        launches.append(a_[6].shape[0])
        return shade(*a_, **k_)
    with monkeypatch.context() as m:
        m.setattr(ops, "env_shade_bounce", counting)
        m.setattr(trace, "ENV_MAX_ENVS", 2)
        split = inference.env_walk(gen, z, b2w, envs[0], **kw)
    assert launches == [2, 2, 1]
    for k in ("image", "shading", "indirect", "transfer", "bounce", "mask"):
        assert torch.equal(_bits(split[k]), _bits(walk[k])), k
    # what a capture launches
    calls = _record_ops(monkeypatch)
    trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED)
    without = list(calls)
    del calls[:]
    trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED, bounces=0)
    zero = list(calls)
    del calls[:]
    trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED, bounces=1)
    one = list(calls)
    assert zero == without
    assert [c for c in zero if c in TRACE_OPS or isinstance(c, tuple)] == [
        "trace_begin", ("march", False), "trace_finish", "sdf_mlp_fwd", "occlusion_ambient_begin", ("march", True), "trace_finish",
        "transfer_resolve", "surface_shade"]
    assert [c for c in one if c in TRACE_OPS or isinstance(c, tuple)] == [
        "trace_begin", ("march", False), "trace_finish", "sdf_mlp_fwd", "occlusion_ambient_begin", ("march", False), "trace_finish"
    ] + (["sdf_mlp_fwd"] if n2 else []) + ["transfer_resolve", "bounce_resolve", "surface_shade"]


CONCAVE_SEED, CONCAVE_POSE = 5, "off"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_capture_of_a_view_that_sees_itself(precision):
    """The golden field of latent 5 is not convex: in the view "off" 47 of its 1952 transfer rays (16 per visible point, f16x3) end
    on the object itself.  Here the second full MLP pass runs, and the bounce map is not zero: the direct transfer is still the
    plain capture's bit for bit, the map is the restatement's on the capture's own states, gradients and albedo, and under a
    constant white environment the indirect light is positive exactly where a ray hit a front face, at most the albedo's
    largest value times the share of those rays."""
    from oi_amd import trace
    from oi_amd.envlight import EnvLight
    gen, z, b2w = G.make_gen(precision, R.R_SOFT), A.latent(CONCAVE_SEED)[0], T.pose(CONCAVE_POSE)
    S = 16
    plain = trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED)
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED, bounces=1)
    assert torch.equal(_bits(cap.transfer), _bits(plain.transfer))
    s = cap.surface
    st, hits = s.transfer_state, s.bounce_hits
    n2 = hits["n_hit"]
    status = st.status.cpu().numpy()
    print(f"envbounce_concave[{precision}] secondary rays that ended HIT", n2, "of", st.N)
    record_margin(f"envbounce_concave[{precision}]", "hit_share", n2 / float(st.N))
    assert n2 == int((status == T.HIT).sum()) >= 10 and cap.stats()["bounce_points"] == n2
    assert hits["grad"].shape == hits["rgb"].shape == hits["hit_points"].shape == (n2, 3)
    slot_np = s.res.hit_slot.cpu().numpy()
    ref, mag, _, front = B.resolve(status, npd(st.rays_d), hits["hit_slot"].cpu().numpy(), npd(hits["grad"]), npd(hits["rgb"]), slot_np,
                                   s.n_hit, S, npd(s.w2b))
    got = npd(cap.bounce).reshape(3, 9, -1)
    bar = B.resolve_bar(mag, S)
    err = np.abs(got - ref)
    record_margin(f"envbounce_concave[{precision}]", "err_over_bar", float((err[bar > 0] / bar[bar > 0]).max()))
    assert (err <= bar).all() and np.abs(got).max() > 0.01
    # the secondary hits are points of the surface: the field's own sdf there is within the trace tolerance
    sdf2 = s.field.sdf(hits["hit_points"])
    assert float(sdf2.abs().max()) <= T.TOL
    out = cap.shade([EnvLight.constant(1)])
    ind = npd(out["indirect"])[0]                                             # (3, H, W)
    lit = np.zeros(s.N, dtype=bool)
    lit[slot_np >= 0] = front.any(0)[slot_np[slot_np >= 0]]
    assert lit.sum() > 0 and (ind.reshape(3, -1)[:, lit] > 0).all() and not ind.reshape(3, -1)[:, ~lit].any()
    share = np.zeros(s.N)
    share[slot_np >= 0] = front.mean(0)[slot_np[slot_np >= 0]]
    assert (ind.reshape(3, -1) <= float(hits["rgb"].max()) * share[None] * (1 + 64 * EPS)).all()
    assert (npd(out["shading"]) - npd(plain.shade([EnvLight.constant(1)])["shading"]) >= 0).all()
