"""Environment lighting on the MI355X (include/oi_envlight.h; oi_amd.envlight; oi_amd.trace.capture_transfer /
render_surface_env; oi_amd.inference.env_walk).  The references: the fp64 restatement tests/helpers/env_ref.py fed the kernels'
own float32 inputs, the already pinned ambient occlusion of include/oi_occlusion.h (under the constant environment the shading
IS the escaped share of the same rays), and an analytic two-sphere scene whose blocked cap is integrated in float64.

Bars (eps = 2^-24):
  oi_env_project       1e-5 sum |w L y| per coefficient: no term passes through more than 128 additions (128 eps = 7.6e-6 of
                       that sum), the rest is room for the float32 weights and basis
  oi_transfer_resolve  (S + 16) eps 1.1 absolute: S accumulated terms of magnitude <= 1.1, 16 for the rotate / normalise /
                       polynomial steps
  oi_transfer_normal   32 eps
  oi_env_shade         16 eps sum_c |T_c L_c|: a 9-term fmaf chain and one product
  analytic scene       5 standard errors of the S = 256 estimator, 5 * 0.5 / sqrt(256) = 0.16 |y|max, against a cap that
                       removes 0.46 |y|max of the +axis lobe (>= 0.3 asked)"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_trace as G
from conftest import record_margin
from helpers import env_ref as E
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
EPS = 2.0 ** -24
N_SET = [1, 63, 64, 65, 257]
ALL_CODES = [T.MISS, T.HIT, T.LIMIT, T.START_INSIDE, T.NONFINITE, T.BACKFACING, T.MARCH, T.REFINE]

_p = lambda t_: None if t_ is None else ctypes.c_void_p(t_.data_ptr())


def _cuda(x, dt=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dt).cuda()


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def _lib():
    from oi_amd import lib, ops
    return lib, lib.load(), ops._stream()


def _w2b(rs):
    """A non-trivial rotation (and a translation nobody may read) as float32 (4, 4)."""
    m = np.eye(4)
    m[:3, :3] = E.random_rotation(rs)
    m[:3, 3] = rs.randn(3)
    return m.astype(np.float32)


def _slots(rs, N, n_hit):
    slot = np.full(N, -1)
    slot[rs.permutation(N)[:n_hit]] = np.arange(n_hit)
    return slot


def _n_hits(N):
    return sorted({0, 1, N - 1, N})


# ---------------------------------------------------------------------------------------------------------------------
# oi_env_project
# ---------------------------------------------------------------------------------------------------------------------
def _project(img):
    lib, L, st = _lib()
    Eenv, _, He, We = img.shape
    rad = guarded_copy(_cuda(img), "radiance")
    nf = L.oi_env_project_partial_floats(Eenv, He, We)
    assert nf == Eenv * -(-He * We // E.PROJECT_CHUNK) * 27
    partial, coeffs = guarded_empty((nf,), what="partial"), guarded_empty((Eenv, 9, 3), what="coeffs")
    assert L.oi_env_project(_p(rad), Eenv, He, We, _p(partial), _p(coeffs), st) == 0
    return coeffs


# the last shape spans three workgroups per map, the third with 32 pixels
@pytest.mark.parametrize("n_env", [1, 3])
@pytest.mark.parametrize("He,We", [(1, 1), (4, 8), (5, 7), (16, 32), (33, 65), (96, 171)])
def test_env_project(He, We, n_env):
    rs = np.random.RandomState(He * 1000 + We * 10 + n_env)
    img = (rs.rand(n_env, 3, He, We) * 4.0 + 0.01).astype(np.float32)
    coeffs = _project(img)
    ref, mag = E.project(img)
    err = np.abs(npd(coeffs) - ref)
    rel = float((err[mag > 0] / mag[mag > 0]).max())                           # (a one-pixel map has coefficients that are 0 exactly)
    case = f"env_project[{He}x{We},E={n_env}]"
    print(case, "error over sum |w L y|", rel)
    record_margin(case, "err_over_abs_sum", rel)
    assert (err <= 1e-5 * mag).all()
    assert torch.equal(_bits(coeffs), _bits(_project(img)))                    # two launches: the same bytes
    for e in range(n_env if n_env > 1 else 0):
        assert torch.equal(_bits(coeffs[e]), _bits(_project(img[e:e + 1])[0])), e   # element e does not depend on E
    from oi_amd import ops
    from oi_amd.envlight import EnvLight
    assert torch.equal(_bits(ops.env_project(_cuda(img))), _bits(coeffs))
    env = EnvLight.from_equirect(np.transpose(img[0], (1, 2, 0)))               # (He, We, 3) on the host
    assert np.array_equal(env.coeffs, npd(coeffs[0]))
    assert np.array_equal(EnvLight.from_equirect(torch.from_numpy(img[0])).coeffs, env.coeffs)       # (3, He, We), a tensor


# ---------------------------------------------------------------------------------------------------------------------
# oi_transfer_resolve / oi_transfer_normal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 16, 256])
@pytest.mark.parametrize("N", N_SET)
def test_transfer_resolve(N, S):
    lib, L, st = _lib()
    bar = (S + 16) * EPS * 1.1
    worst = 0.0
    for n_hit in _n_hits(N):
        rs = np.random.RandomState(N * 1000 + S * 7 + n_hit)
        Q = S * n_hit
        d = A.unit(rs.randn(Q, 3)).astype(np.float32)
        status = rs.choice(ALL_CODES, size=Q, p=[0.44] + [0.08] * 7).astype(np.uint8)
        slot_np, w2b_np = _slots(rs, N, n_hit), _w2b(rs)
        slot, w2b = guarded_copy(_cuda(slot_np, torch.int32), "hit_slot"), guarded_copy(_cuda(w2b_np), "w2b")
        st_t = guarded_copy(_cuda(status, torch.uint8), "status") if n_hit else None
        d_t = guarded_copy(_cuda(d), "rays_d") if n_hit else None
        outs = []
        for _ in range(2):
            out = guarded_empty((9, N), what="transfer")
            assert L.oi_transfer_resolve(_p(st_t), _p(d_t), _p(slot), N, n_hit, S, _p(w2b), _p(out), st) == 0
            outs.append(out)
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
        ref = E.transfer(status, d, slot_np, n_hit, S, w2b_np)
        got = npd(outs[0])
        worst = max(worst, float(np.abs(got - ref).max()))
        assert np.abs(got - ref).max() <= bar, (n_hit, np.abs(got - ref).max(), bar)
        assert not got[:, slot_np < 0].any()                                      # exact zeros off the mask
        if n_hit:
            from oi_amd import ops
            assert torch.equal(_bits(ops.transfer_resolve(st_t, d_t, slot, N, n_hit, S, w2b)), _bits(outs[0]))
    print(f"transfer_resolve[N={N},S={S}] worst", worst, "bar", bar)
    record_margin(f"transfer_resolve[N={N},S={S}]", "err_over_bar", worst / bar)


@pytest.mark.parametrize("N", N_SET)
def test_transfer_normal(N):
    lib, L, st = _lib()
    bar = 32 * EPS
    for n_hit in _n_hits(N):
        rs = np.random.RandomState(N * 10 + n_hit)
        grad = (rs.randn(n_hit, 3) * rs.uniform(0.2, 3.0, (n_hit, 1))).astype(np.float32)
        if n_hit >= 2:
            grad[1] = 0.0                                                          # below the 1e-6 of the normalisation: n = 0
        slot_np, w2b_np = _slots(rs, N, n_hit), _w2b(rs)
        slot, w2b = guarded_copy(_cuda(slot_np, torch.int32), "hit_slot"), guarded_copy(_cuda(w2b_np), "w2b")
        g_t = guarded_copy(_cuda(grad), "grad") if n_hit else None
        out = guarded_empty((9, N), what="transfer")
        assert L.oi_transfer_normal(_p(g_t), _p(slot), N, n_hit, _p(w2b), _p(out), st) == 0
        ref = E.transfer_normal(grad, slot_np, w2b_np)
        err = float(np.abs(npd(out) - ref).max())
        record_margin(f"transfer_normal[N={N}]", "err_over_bar", err / bar)
        assert err <= bar, (n_hit, err)
        assert not npd(out)[:, slot_np < 0].any()
        if n_hit:
            from oi_amd import ops
            assert torch.equal(_bits(ops.transfer_normal(g_t, slot, N, n_hit, w2b)), _bits(out))


# ---------------------------------------------------------------------------------------------------------------------
# oi_env_shade
# ---------------------------------------------------------------------------------------------------------------------
def _shade(lib, L, st, N, n_hit, F, status, slot, rgb, transfer, envs, bg, want=("shading", "image")):
    P = lib.EnvShadeParams()
    P.N, P.n_hit, P.F = N, n_hit, F
    out = {k: guarded_empty((F, 3, N), what=k) for k in want}
    for k_, v_ in dict(status=status, hit_slot=slot, rgb=rgb, transfer=transfer, envs=envs, bg=bg, shading=out.get("shading"),
                       image=out.get("image")).items():
        setattr(P, k_, _p(v_))
    assert L.oi_env_shade(ctypes.byref(P), st) == 0
    return out


@pytest.mark.parametrize("F", [1, 2, 256])
@pytest.mark.parametrize("N", N_SET)
def test_env_shade(N, F):
    lib, L, st = _lib()
    for n_hit in sorted({0, max(1, N - 1)}):
        rs = np.random.RandomState(N * 1000 + F + n_hit)
        slot_np = _slots(rs, N, n_hit)
        mask = slot_np >= 0
        status_np = np.where(mask, T.HIT, rs.choice([T.MISS, T.LIMIT, T.START_INSIDE, T.NONFINITE], size=N)).astype(np.uint8)
        tr_np = rs.uniform(-1, 1, (9, N)).astype(np.float32)                      # non-zero off the mask too: the kernel masks
        env_np = rs.randn(F, 9, 3).astype(np.float32)
        if n_hit:
            env_np[0, :, 0] = -tr_np[:, np.nonzero(mask)[0][0]]                    # a pixel whose shading is -|T|^2 < 0
        rgb_np, bg_np = rs.rand(n_hit, 3).astype(np.float32), np.array([0.1, 0.2, 0.3], dtype=np.float32)
        status, slot = guarded_copy(_cuda(status_np, torch.uint8), "status"), guarded_copy(_cuda(slot_np, torch.int32), "hit_slot")
        rgb = guarded_copy(_cuda(rgb_np), "rgb") if n_hit else None
        transfer, envs, bg = guarded_copy(_cuda(tr_np), "transfer"), guarded_copy(_cuda(env_np), "envs"), guarded_copy(_cuda(bg_np), "bg")
        out = _shade(lib, L, st, N, n_hit, F, status, slot, rgb, transfer, envs, bg)
        alb = np.zeros((N, 3))
        alb[mask] = rgb_np[slot_np[mask]]
        sh, img, mag = E.shade(tr_np, env_np, mask, alb, bg_np)
        bar = 16 * EPS * mag
        e_sh, e_img = np.abs(npd(out["shading"]) - sh), np.abs(npd(out["image"]) - img)
        if n_hit:
            record_margin(f"env_shade[N={N},F={F}]", "err_over_bar", float((e_sh / bar)[:, :, mask].max()))
        assert (e_sh <= bar).all() and (e_img <= bar).all()
        # off the mask: shading 0, image the background, exactly
        assert not npd(out["shading"])[:, :, ~mask].any()
        assert np.array_equal(npd(out["image"])[:, :, ~mask], np.broadcast_to(bg_np.astype(np.float64)[None, :, None], (F, 3, int((~mask).sum()))))
        if n_hit:
            neg = npd(out["shading"])[:, :, mask] < 0
            assert neg.any() and not npd(out["image"])[:, :, mask][neg].any()     # clamped in the image, kept in the shading
        # no background given: black
        black = _shade(lib, L, st, N, n_hit, F, status, slot, rgb, transfer, envs, None, want=("image",))
        assert not npd(black["image"])[:, :, ~mask].any() and torch.equal(black["image"][:, :, _cuda(mask, torch.bool)],
                                                                           out["image"][:, :, _cuda(mask, torch.bool)])
        # either output may be absent
        only_s = _shade(lib, L, st, N, n_hit, F, status, slot, rgb, transfer, envs, bg, want=("shading",))
        only_i = _shade(lib, L, st, N, n_hit, F, status, slot, rgb, transfer, envs, bg, want=("image",))
        assert torch.equal(_bits(only_s["shading"]), _bits(out["shading"])) and torch.equal(_bits(only_i["image"]), _bits(out["image"]))
        # result f of the F-environment launch is the 1-environment launch of environment f, bit for bit
        for f in sorted({0, F // 3, F - 1}):
            one = _shade(lib, L, st, N, n_hit, 1, status, slot, rgb, transfer, guarded_copy(_cuda(env_np[f:f + 1]), "env1"), bg)
            for k in ("shading", "image"):
                assert torch.equal(_bits(one[k][0]), _bits(out[k][f])), (k, f)
        from oi_amd import ops
        via = ops.env_shade(status, slot, rgb, n_hit, transfer, envs, bg)
        for k in ("shading", "image"):
            assert torch.equal(_bits(via[k]), _bits(out[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the golden field
# ---------------------------------------------------------------------------------------------------------------------
SEED, POSE = R.SOFT_VIEWS[0]
BG = (0.1, 0.2, 0.3)


def _view(precision):
    return G.make_gen(precision, R.R_SOFT), A.latent(SEED)[0], T.pose(POSE)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_constant_environment_is_the_ambient_occlusion(precision):
    """(a) the same rays as render_surface's ambient occlusion at distance 4, and T_0 * 2 sqrt(pi) is the escaped share."""
    from oi_amd import trace
    from oi_amd.envlight import EnvLight
    gen, z, b2w = _view(precision)
    k = R.SEED
    out = trace.render_surface_env(gen, z, b2w, envs=[EnvLight.constant(1)], transfer_samples=16, seed=k, bg=BG)
    ref = trace.render_surface(gen, z, b2w, ao_samples=16, ao_distance=4.0, seed=k)
    H = R.R_SOFT
    assert out["shading"].shape == out["image"].shape == (1, 3, H, H) and out["transfer"].shape == (1, 9, H, H)
    mask = out["mask"][0, 0] > 0
    n_hit = int(mask.sum())
    assert n_hit > 50 and out["stats"]["hit"] == n_hit and out["stats"]["transfer_evals"] > 0
    sh, ao = out["shading"][:, 0], ref["ambient_occlusion"][:, 0]
    err = float((sh - ao)[:, mask].abs().max())
    print(f"envlight_identity[{precision}] shading against ambient occlusion", err, "escaped share", float(ao[:, mask].mean()))
    record_margin(f"envlight_identity[{precision}]", "shading_vs_ao", err)
    assert err <= 4 * EPS
    assert torch.equal(out["shading"][0, 1], out["shading"][0, 0]) and torch.equal(out["shading"][0, 2], out["shading"][0, 0])
    # off the mask the shading is 0 and the image is bg; on it the image is max(shading, 0) albedo
    assert not bool(out["shading"][:, :, ~mask].any())
    bg = torch.tensor(BG).cuda()
    assert torch.equal(out["image"][0][:, ~mask], bg[:, None].expand(3, int((~mask).sum())))
    assert torch.equal(out["image"][0][:, mask], (out["shading"][0].clamp(min=0) * out["albedo"][0])[:, mask])
    # the G-buffer is render_surface's, and so are the rays
    for key in ("depth", "position", "normal_map", "normal_object", "albedo", "mask"):
        assert torch.equal(_bits(out[key]), _bits(ref[key])), key
    assert set(out) == {"depth", "position", "normal_map", "normal_object", "albedo", "mask", "image", "shading", "transfer",
                        "transfer_trace", "stats", "trace"}
    a, b = out["transfer_trace"], ref["ao_trace"]
    pa, pb = out["trace"].hit_index.long(), ref["trace"].hit_index.long()       # the slots of two primary traces may differ
    order_a, order_b = torch.argsort(pa), torch.argsort(pb)
    assert torch.equal(pa[order_a], pb[order_b])
    assert torch.equal(a.status.view(16, n_hit)[:, order_a], b.status.view(16, n_hit)[:, order_b])
    assert torch.equal(a.rays_d.view(16, n_hit, 3)[:, order_a], b.rays_d.view(16, n_hit, 3)[:, order_b])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_transfer_map_against_the_restatement(precision):
    """(b) the map of a capture against the restatement fed the state's own rays_d and status."""
    from oi_amd import trace
    gen, z, b2w = _view(precision)
    S = 16
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples=S, seed=R.SEED)
    s = cap.surface
    st = s.transfer_state
    assert st.N == S * s.n_hit and int(st.status.max()) <= T.BACKFACING
    ref = E.transfer(st.status.cpu().numpy(), npd(st.rays_d), s.res.hit_slot.cpu().numpy(), s.n_hit, S, npd(s.w2b))
    err = float(np.abs(npd(cap.transfer).reshape(9, -1) - ref).max())
    bar = (S + 16) * EPS * 1.1
    record_margin(f"envlight_transfer[{precision}]", "err_over_bar", err / bar)
    print(f"envlight_transfer[{precision}] error", err, "bar", bar)
    assert err <= bar
    assert cap.stats()["transfer_evals"] == s.transfer_evals > 0 and cap.maps["mask"].shape == (1, 1, R.R_SOFT, R.R_SOFT)
    # the directional part carries information: the +normal lobe is positive on the mask
    nw = npd(cap.maps["normal_map"])[0].reshape(3, -1)
    t = npd(cap.transfer).reshape(9, -1)
    lobe = (t[[3, 1, 2]] * nw).sum(0)[npd(cap.maps["mask"]).reshape(-1) > 0]        # (y3, y1, y2) ~ (x, y, z)
    assert (lobe > 0).mean() > 0.9


@pytest.mark.parametrize("precision", PRECISIONS)
def test_env_walk(precision, monkeypatch):
    """(c) a walk is one capture shaded under host-rotated environments, whatever the split into launches."""
    from oi_amd import inference, ops, trace
    from oi_amd.envlight import EnvLight
    gen, z, b2w = _view(precision)
    env = EnvLight(np.random.RandomState(2).randn(9, 3) * 0.5 + np.eye(9)[0][:, None] * 3.0)
    kw = dict(n_frames=5, axis=(0.2, -0.1, 1.0), transfer_samples=4, seed=R.SEED, bg=BG)
    walk = inference.env_walk(gen, z, b2w, env, **kw)
    H = R.R_SOFT
    assert walk["image"].shape == walk["shading"].shape == (5, 3, H, H) and walk["transfer"].shape == (1, 9, H, H)
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples=4, seed=R.SEED)
    assert torch.equal(cap.transfer, walk["transfer"])
    for i, Rm in enumerate(inference.env_walk_rotations(5, kw["axis"])):
        one = cap.shade([env.rotated(Rm)], bg=BG)
        assert torch.equal(_bits(one["image"][0]), _bits(walk["image"][i])), i
        assert torch.equal(_bits(one["shading"][0]), _bits(walk["shading"][i])), i
    assert not torch.equal(walk["shading"][0], walk["shading"][2])               # the environment is not symmetric
    launches = []
    shade = ops.env_shade

    def counting(*a, **k):
        launches.append(a[5].shape[0])
        return shade(*a, **k)
    monkeypatch.setattr(ops, "env_shade", counting)
    monkeypatch.setattr(trace, "ENV_MAX_ENVS", 2)
    split = inference.env_walk(gen, z, b2w, env, **kw)
    assert launches == [2, 2, 1]
    for k in ("image", "shading", "transfer", "mask"):
        assert torch.equal(_bits(split[k]), _bits(walk[k])), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_samples_takes_the_closed_form(precision, monkeypatch):
    """(d) transfer_samples = 0 traces nothing and is the unshadowed transfer of the normal."""
    from oi_amd import ops, trace
    from oi_amd.envlight import EnvLight

    def refuse(*a, **k):
        raise AssertionError("a secondary trace ran with transfer_samples = 0")
    monkeypatch.setattr(ops, "occlusion_ambient_begin", refuse)
    monkeypatch.setattr(ops, "transfer_resolve", refuse)
    gen, z, b2w = _view(precision)
    out = trace.render_surface_env(gen, z, b2w, envs=[EnvLight.constant(1)], transfer_samples=0)
    assert out["stats"]["transfer_evals"] == 0 and out["transfer_trace"] is None
    mask = out["mask"][0, 0] > 0
    err = float((out["shading"][0][:, mask] - 1.0).abs().max())
    record_margin(f"envlight_closed_form[{precision}]", "shading_minus_one", err)
    assert int(mask.sum()) > 50 and err <= 8 * EPS
    assert not bool(out["shading"][:, :, ~mask].any()) and not bool(out["image"][:, :, ~mask].any())   # no bg: black
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples=0)
    s = cap.surface
    ref = E.transfer_normal(npd(s.grad), s.res.hit_slot.cpu().numpy(), npd(s.w2b))
    assert np.abs(npd(cap.transfer).reshape(9, -1) - ref).max() <= 32 * EPS
    # the closed form's band 1 is 2/3 k1 times the world normal of the G-buffer
    nw = npd(cap.maps["normal_map"])[0].reshape(3, -1)
    t = npd(cap.transfer).reshape(9, -1)
    assert np.abs(t[[3, 1, 2]] - (2.0 / 3.0) * E.Y_MAX_BAND1 * nw).max() <= 32 * EPS


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene, through the C ABI on guarded buffers, the field evaluated by torch between the steps
# ---------------------------------------------------------------------------------------------------------------------
def _two_spheres(pts):
    c0, c1 = (torch.tensor(c, dtype=torch.float32, device=pts.device) for c in (E.C0, E.C1))
    return torch.minimum((pts - c0).norm(dim=-1) - E.R0, (pts - c1).norm(dim=-1) - E.R1)


def _guarded_state(Q, tag):
    """An oi_trace_state of Q rays on guarded, poisoned buffers (the int16 step counts and the partly written lists carry
    guards only)."""
    from oi_amd import lib
    g = lambda sh, dt=torch.float32, what="?", mw=True: guarded_empty(sh, dt, what=f"{tag}_{what}", must_write=mw)
    arr = dict(rays_o=g((Q, 3), what="rays_o"), rays_d=g((Q, 3), what="rays_d"), near_=g((Q,), what="near"), far_=g((Q,), what="far"),
               t=g((Q,), what="t"), status=g((Q,), torch.uint8, "status"), steps=g((Q,), torch.int16, "steps", False),
               bracket=g((Q, 4), what="bracket"), side=g((Q,), torch.uint8, "side"), active=g((2, Q), torch.int32, "active", False),
               points=g((Q, 3), what="points", mw=False), counts=g((lib.TRACE_COUNT_WORDS,), torch.int32, "counts"))
    S = lib.TraceState()
    S.N = Q
    for k_, v_ in arr.items():
        setattr(S, k_, _p(v_))
    return arr, S


def _anyhit_loop(arr, S, field, max_steps):
    """oi_occlusion_step until no ray is in flight, then oi_trace_finish.  -> steps run."""
    lib, L, st = _lib()
    Q = S.N
    bound, k = int(arr["counts"][0].item()), 0
    while bound > 0 and k < max_steps:
        sdf = guarded_copy(field(arr["points"][:bound]), "sdf")
        assert L.oi_occlusion_step(ctypes.byref(S), _p(sdf), bound, k, T.TOL, T.OMEGA, st) == 0
        k += 1
        bound = int(arr["counts"][k].item())
    hit_index = guarded_empty((Q,), torch.int32, what="f_hit_index", must_write=False)
    hit_points = guarded_empty((Q, 3), what="f_hit_points", must_write=False)
    hit_slot = guarded_empty((Q,), torch.int32, what="f_hit_slot")
    assert L.oi_trace_finish(ctypes.byref(S), _p(hit_index), _p(hit_points), _p(hit_slot), st) == 0
    return k


def test_analytic_blocked_cap():
    """Three pixels at the point on top of the lower sphere, directly under the upper one, and one on the lower sphere's
    equator, which sees nothing.  In the axis frame (w2b = identity) the +axis lobe T_2 under the blocker is the unoccluded
    closed form 2/3 k1 = 0.326 minus the cap's contribution 0.459 k1 = 0.224; the bar is 5 standard errors of the S = 256
    estimator, 5 * 0.5 / sqrt(256) k1 = 0.156 k1 = 0.076: a third of the effect."""
    lib, L, st = _lib()
    S, k0, k1 = 256, 0.5 / np.sqrt(np.pi), E.Y_MAX_BAND1
    alpha = E.analytic_cap_angle()
    cap = E.cap_transfer(alpha)
    bar = 5 * 0.5 / np.sqrt(S)
    assert cap[2] >= 0.3 * k1 > bar * k1
    pts = np.array([[0.0, 0.0, E.R0]] * 3 + [[E.R0, 0.0, 0.0]])
    nrm = pts / E.R0
    n_hit, pix = 4, np.array([11, 4, 300, 77])
    hp, grad = guarded_copy(_cuda(pts), "hit_points"), guarded_copy(_cuda(nrm * 1.7), "grad")
    hit_index = guarded_copy(_cuda(pix, torch.int32), "hit_index")
    arr, St = _guarded_state(S * n_hit, "env")
    assert L.oi_occlusion_ambient_begin(ctypes.byref(St), _p(hp), _p(grad), _p(hit_index), n_hit, S, T.BIAS, 4.0, R.SEED, st) == 0
    assert int(arr["counts"][0].item()) == S * n_hit
    T.assert_secondary_begin_state(arr)
    steps = _anyhit_loop(arr, St, _two_spheres, 256)
    status = arr["status"].cpu().numpy().reshape(S, n_hit)
    assert status.max() <= T.NONFINITE and (status[:, 3] == T.MISS).all()         # the equator sees nothing
    slot_np = np.array([2, -1, 0, 1, 3])
    slot, w2b = guarded_copy(_cuda(slot_np, torch.int32), "hit_slot"), guarded_copy(torch.eye(4).cuda(), "w2b")
    out = guarded_empty((9, 5), what="transfer")
    assert L.oi_transfer_resolve(_p(arr["status"]), _p(arr["rays_d"]), _p(slot), 5, n_hit, S, _p(w2b), _p(out), st) == 0
    t = npd(out)
    ref = E.transfer(arr["status"].cpu().numpy(), npd(arr["rays_d"]), slot_np, n_hit, S, np.eye(4))
    assert np.abs(t - ref).max() <= (S + 16) * EPS * 1.1 and not t[:, 1].any()
    # where the occlusion is real: T_0 * 2 sqrt(pi) is oi_occlusion_resolve's escaped share of the same states (the resolve bar
    # on T_0, scaled by 2 sqrt(pi))
    share = guarded_empty((1, 5), what="share")
    assert L.oi_occlusion_resolve(_p(arr["status"]), _p(slot), 5, n_hit, 1, S, _p(share), st) == 0
    on = slot_np >= 0
    assert np.abs(t[0] * 2.0 * np.sqrt(np.pi) - npd(share)[0])[on].max() <= (S + 16) * EPS * 1.1 * 2.0 * np.sqrt(np.pi)
    assert 0.4 < npd(share)[0, 0] < 0.5                                           # 1 - sin^2(0.826) = 0.459 of the rays escape
    open_top = E.closed_form(np.array([0.0, 0.0, 1.0]))
    expect = open_top - cap
    under = t[:, [2, 3, 0]]                                                       # the pixels of slots 0, 1, 2
    print("analytic cap: half-angle", alpha, "steps", steps, "T_2 under the blocker", under[2], "expected", expect[2], "unoccluded",
          open_top[2], "bar", bar * k1, "occluded share", (status[:, :3] != T.MISS).mean(0), "expected", np.sin(alpha) ** 2)
    record_margin("envlight_analytic_cap", "T2_err_over_bar", float(np.abs(under[2] - expect[2]).max() / (bar * k1)))
    assert (np.abs(under[2] - expect[2]) <= bar * k1).all()
    assert (np.abs(under[0] - expect[0]) <= bar * k0).all()                       # the escaped share, 1 - sin^2(alpha), times y_0
    assert (under[2] < open_top[2] - (cap[2] - bar * k1)).all()                   # and it is below the unoccluded lobe
    # the equator pixel: the unoccluded estimator about +x
    assert abs(t[3, 4] - (2.0 / 3.0) * k1) <= bar * k1 and abs(t[0, 4] - k0) <= (S + 16) * EPS
