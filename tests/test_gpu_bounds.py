"""Kernels at the shapes where tails break, every buffer guarded (tests/helpers/guarded.py).

Each case calls the C ABI (or an oi_amd.ops wrapper whose outputs the `guarded_ops` fixture guards) with inputs copied
into input-guarded arenas, outputs and scratch in poisoned, guarded arenas -- scratch and workspace at EXACTLY the size
their sizing export returns -- and compares with a plain high-precision reference at the bar the existing test of that
kernel uses (cited per case).  At teardown the fixture fails the case on any store outside a buffer, any output element
never written, any write to an input.  tests/test_bounds_coverage_cpu.py keeps every writing export of include/oi_hip.h
named here (or exempted there, with the reason)."""
import ctypes
import math
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oi_oracle as O
from conftest import load_golden, maxdiff
from helpers import mc_numpy as M
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "bf16x6": 3, "f16x3": 4}


def _L():
    from oi_amd import lib
    return lib.load()


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    from oi_amd import lib
    lib.check(rc, what)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


@pytest.fixture(scope="module")
def packs(sdf_sd, col_sd):
    from oi_amd import ops
    from oi_amd.params import stack_field_params
    P = stack_field_params({k: v.cuda() for k, v in sdf_sd.items()}, {k: v.cuda() for k, v in col_sd.items()})
    out = {m: ops.mlp_pack_weights(P["w0"], P["b0"], P["wh"], P["bh"], P["wsig"], P["bsig"], P["wv"], P["bv"], P["wrgb"],
                                   P["brgb"], p) for m, p in PREC.items()}
    return P, out


def _film(P, w):
    """gamma / beta [B][9][128] from w (fp32 on the device, the kernels' own input)."""
    from oi_amd import ops
    _, gamma, beta = ops.film_params(P["style_w"], P["style_b"], P["gw"], P["gb"], P["bw"], P["bb"], w=w.cuda())
    return gamma, beta


def _d_w_from_film(P, d_gamma, d_beta, layers):
    """d L / d w through gamma = 15 (w Wg^T + bg) + 30, beta = 0.25 (w Wb^T + bb) (include/oi_hip.h oi_film_params), fp64:
    the way every d_gamma / d_beta entry is compared with the oracle's gradient with respect to the style vector."""
    gw, bw = P["gw"].double().cpu(), P["bw"].double().cpu()
    dg, db = d_gamma.double().cpu(), d_beta.double().cpu()
    return sum(15.0 * dg[:, l] @ gw[l] + 0.25 * db[:, l] @ bw[l] for l in layers)


# ---------------------------------------------------------------------------------------------------------------------
# 1. MLP forward: five precisions x four output sets x ragged point counts (oi_sdf_mlp_fwd, oi_mlp_scratch_bytes_prec)
# ---------------------------------------------------------------------------------------------------------------------
# bars: tests/test_gpu_kernels.py::test_sdf_mlp_golden (sdf, relative grad, rgb) and its feature bars
FWD_TOL = {"f32": (2e-5, 1e-4, 2e-5, 1e-4), "bf16x6": (2e-5, 1e-4, 2e-5, 1e-4), "f16x3": (2e-5, 1e-4, 2e-5, 1e-4),
           "bf16x3": (5e-5, 2e-4, 5e-5, 3e-4), "bf16": (3e-2, 1.5e-1, 3e-2, 1e-1)}
OUTSETS = {"sdf": (False, False, False), "grad": (True, False, False), "grad_rgb": (True, True, False),
           "grad_rgb_feat": (True, True, True)}


@lru_cache(maxsize=None)
def _fwd_case(n, B):
    """Seeded points / style vectors and the fp64 oracle's sdf, feature, gradient and albedo."""
    from conftest import load_golden as lg
    sd = {k: v.double() for k, v in lg("weights_sdf").items()}
    csd = {k: v.double() for k, v in lg("weights_color").items()}
    g = torch.Generator().manual_seed(1000 * B + n)
    pts = torch.rand(B * n, 3, generator=g) * 2.4 - 1.2
    w = O.style_mlp({k: v.float() for k, v in sd.items()}, torch.randn(B, 64, generator=g))
    sdf, feat, grad = O.sdf_forward(sd, pts.double(), w.double(), want_grad=True)
    rgb = O.color_head(csd, feat, grad, w.double())
    return pts, w, sdf.squeeze(-1), feat, grad, rgb


def _mlp_fwd_guarded(gs, pts, packed, gamma, beta, B, n, mode, want_grad, want_rgb, want_feat, flags=0, scratch=None):
    L = _L()
    prec = PREC[mode]
    dev = "cuda"
    pts_g, packed_g, gamma_g, beta_g = (gs.copy(t.cuda(), f"oi_sdf_mlp_fwd input {nm}") for t, nm in
                                        ((pts, "pts"), (packed, "packed"), (gamma, "gamma"), (beta, "beta")))
    sdf = gs.empty((B * n,), torch.float32, dev, f"oi_sdf_mlp_fwd[{mode}] sdf")
    grad = gs.empty((B * n, 3), torch.float32, dev, f"oi_sdf_mlp_fwd[{mode}] grad") if want_grad else None
    rgb = gs.empty((B * n, 3), torch.float32, dev, f"oi_sdf_mlp_fwd[{mode}] rgb") if want_rgb else None
    feat = gs.empty((B * n, 128), torch.float32, dev, f"oi_sdf_mlp_fwd[{mode}] feat") if want_feat else None
    if want_grad and scratch is None:
        scratch = gs.scratch(L.oi_mlp_scratch_bytes_prec(B, n, prec), dev, f"oi_sdf_mlp_fwd[{mode}] scratch")
    fast = int(mode == "bf16")
    if flags:
        ok(L.oi_sdf_mlp_fwd_ex(vp(pts_g), vp(packed_g), vp(gamma_g), vp(beta_g), vp(sdf), vp(grad), vp(rgb), vp(feat), vp(scratch),
                               B, n, prec, fast, flags, stream()), "oi_sdf_mlp_fwd_ex")
    else:
        ok(L.oi_sdf_mlp_fwd(vp(pts_g), vp(packed_g), vp(gamma_g), vp(beta_g), vp(sdf), vp(grad), vp(rgb), vp(feat),
                            vp(scratch) if want_grad else None, B, n, prec, fast, stream()), "oi_sdf_mlp_fwd")
    return sdf, grad, rgb, feat


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 127, 129, 257])
@pytest.mark.parametrize("outs", list(OUTSETS))
@pytest.mark.parametrize("mode", list(PREC))
def test_mlp_forward_ragged(guarded_ops, packs, mode, outs, n, B):
    P, pk = packs
    pts, w, sdf_o, feat_o, grad_o, rgb_o = _fwd_case(n, B)
    gamma, beta = _film(P, w)
    want_grad, want_rgb, want_feat = OUTSETS[outs]
    sdf, grad, rgb, feat = _mlp_fwd_guarded(guarded_ops, pts, pk[mode], gamma, beta, B, n, mode, want_grad, want_rgb, want_feat)
    t_sdf, t_grad, t_rgb, t_feat = FWD_TOL[mode]
    assert maxdiff(sdf.cpu(), sdf_o) < t_sdf
    if want_grad:
        assert maxdiff(grad.cpu(), grad_o) < t_grad * max(1.0, float(grad_o.abs().max()))
    if want_rgb:
        assert maxdiff(rgb.cpu(), rgb_o) < t_rgb
    if want_feat:
        assert maxdiff(feat.cpu(), feat_o) < t_feat


def test_mlp_forward_blob_ready_ragged(guarded_ops, packs, sdf_sd):
    """OI_MLP_BLOB_READY (oi_sdf_mlp_fwd_ex): the per-element blobs written by oi_prep_render into a guarded scratch of exactly
    oi_mlp_scratch_bytes_prec(B, n, F16X3) bytes, then the forward at a ragged n -- bit-identical to the plain call
    (oi_hip.h: "the bytes are the same") and within the f16x3 bars of the oracle."""
    from oi_amd import lib, ops
    L = _L()
    gs = guarded_ops
    P, pk = packs
    B, n, R, S = 3, 129, 2, 3
    pts, w, sdf_o, feat_o, grad_o, rgb_o = _fwd_case(n, B)
    g = torch.Generator().manual_seed(7)
    z = torch.randn(B, 64, generator=g)
    w_z = O.style_mlp(sdf_sd, z)
    scratch = gs.scratch(L.oi_mlp_scratch_bytes_prec(B, n, PREC["f16x3"]), "cuda", "oi_sdf_mlp_fwd_ex scratch")
    off = L.oi_mlp_f3_blob_offset(B, n)
    blob = scratch[off:off + B * L.oi_mlp_f3_blob_bytes()]
    eye = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    eye[:, 2, 3] = -3.0
    film = {k: P[k] for k in ("style_w", "style_b", "gw", "gb", "bw", "bb")}
    out = ops.prep_render(eye, eye, eye, np.zeros((B, 2), np.float32), np.zeros((B, 3), np.float32),
                          torch.eye(3, device="cuda"), R, S, None, torch.tensor([0.3, -0.5, -0.8]).cuda(), film, z.cuda(), f3_packed=pk["f16x3"], f3_blob=blob)
    a = _mlp_fwd_guarded(gs, pts, pk["f16x3"], out["gamma"], out["beta"], B, n, "f16x3", True, True, True,
                         flags=lib.OI_MLP_BLOB_READY, scratch=scratch)
    b = _mlp_fwd_guarded(gs, pts, pk["f16x3"], out["gamma"], out["beta"], B, n, "f16x3", True, True, True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    sdf_z, feat_z, grad_z = O.sdf_forward(sdf_sd, pts, w_z, want_grad=True)
    assert maxdiff(a[0].cpu(), sdf_z.squeeze(-1)) < 2e-5
    assert maxdiff(a[1].cpu(), grad_z) < 1e-4 * max(1.0, float(grad_z.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# 2. MLP backward (oi_sdf_mlp_bwd, oi_sdf_mlp_bwd_feat; oi_mlp_bwd_scratch_bytes_capped)
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_mlp_grads(pts, w, cs, cg, cr, cf=None):
    """fp64 autograd through the oracle: d L / d (parameters, w), L = <cs, sdf> + <cg, grad> + <cr, rgb> [+ <cf, feat>]."""
    sd = {k: v.double().requires_grad_(True) for k, v in load_golden("weights_sdf").items()}
    csd = {k: v.double().requires_grad_(True) for k, v in load_golden("weights_color").items()}
    wd = w.double().clone().requires_grad_(True)
    sdf, feat, grad = O.sdf_forward(sd, pts.double(), wd, want_grad=True)
    rgb = O.color_head(csd, feat, grad, wd)
    loss = (sdf.squeeze(-1) * cs.double()).sum() + (grad * cg.double()).sum() + (rgb * cr.double()).sum()
    if cf is not None:
        loss = loss + (feat * cf.double()).sum()
    names = [k for k in sd if not k.startswith("style.")]
    gr = torch.autograd.grad(loss, [sd[k] for k in names] + list(csd.values()) + [wd])
    out = dict(zip(["sdf." + k for k in names] + ["col." + k for k in csd] + ["w"], gr))
    return out


def _unpack_bwd(d_small, d_wmat):
    """The parameter gradients in the reference's names from the packed layout of include/oi_hip.h (oi_sdf_mlp_bwd)."""
    s = d_small.double().cpu()
    m = d_wmat.double().cpu()
    o = {"sdf.pts_linears.0.weight": s[0:384].view(128, 3)}
    db = s[384:1536].view(9, 128)
    for l in range(8):
        o[f"sdf.pts_linears.{l}.bias"] = db[l]
        if l:
            o[f"sdf.pts_linears.{l}.weight"] = m[l - 1]
    o["col.views_linears.bias"] = db[8]
    o["sdf.sigma_linear.weight"] = s[1536:1664].view(1, 128)
    o["sdf.sigma_linear.bias"] = s[1664:1665]
    o["col.views_linears.weight"] = torch.cat([m[7], s[1668:2052].view(128, 3)], 1)
    o["col.rgb_linear.weight"] = s[2052:2436].view(3, 128)
    o["col.rgb_linear.bias"] = s[2436:2439]
    return o


# bar: tests/test_gpu_backward.py::test_mlp_backward_vs_oracle (f32 / f16x3: 2e-5 relative to each tensor's largest entry)
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n,cap_tiles,feat", [(1, None, False), (129, None, False), (129, None, True), (300, 1, False)])
def test_mlp_backward_ragged(guarded_ops, packs, mode, n, B, cap_tiles, feat):
    """cap_tiles = 1: a scratch of one 128-point tile per element, so the 300 points run in chunks of 128, 128, 44 -- the last
    one ending inside a tile."""
    L = _L()
    gs = guarded_ops
    P, pk = packs
    assert L.oi_mlp_bwd_small_floats() == 2440
    pts, w, *_ = _fwd_case(n, B)
    g = torch.Generator().manual_seed(n + 7 * B)
    cs, cg, cr = torch.randn(B * n, generator=g), 0.1 * torch.randn(B * n, 3, generator=g), torch.randn(B * n, 3, generator=g)
    cf = 0.05 * torch.randn(B * n, 128, generator=g) if feat else None
    ref = _oracle_mlp_grads(pts, w, cs, cg, cr, cf)
    gamma, beta = _film(P, w)
    sdf, grad, rgb, feat_f = _mlp_fwd_guarded(gs, pts, pk[mode], gamma, beta, B, n, mode, True, True, True)
    cap = L.oi_mlp_bwd_scratch_bytes(B, 128) * cap_tiles if cap_tiles else L.oi_mlp_bwd_scratch_bytes(B, n)
    nbytes = L.oi_mlp_bwd_scratch_bytes_capped(B, n, cap)
    if cap_tiles:
        assert nbytes == cap and nbytes < L.oi_mlp_bwd_scratch_bytes(B, n)
    scratch = gs.scratch(nbytes, "cuda", f"oi_sdf_mlp_bwd[{mode}] scratch")
    d_small = gs.zeros((L.oi_mlp_bwd_small_floats(),), torch.float32, "cuda", "oi_sdf_mlp_bwd d_small")
    d_wmat = gs.zeros((8, 128, 128), torch.float32, "cuda", "oi_sdf_mlp_bwd d_wmat")
    d_gamma = gs.zeros((B, 9, 128), torch.float32, "cuda", "oi_sdf_mlp_bwd d_gamma")
    d_beta = gs.zeros((B, 9, 128), torch.float32, "cuda", "oi_sdf_mlp_bwd d_beta")
    ins = [gs.copy(t.cuda().contiguous(), f"oi_sdf_mlp_bwd input {nm}") for t, nm in
           ((pts, "pts"), (pk[mode], "packed"), (gamma, "gamma"), (beta, "beta"), (grad, "grad_fwd"), (rgb, "rgb_fwd"),
            (feat_f, "feat_fwd"), (cs, "g_sdf"), (cg, "g_grad"), (cr, "g_rgb"))]
    outs = [vp(d_small), vp(d_wmat), vp(d_gamma), vp(d_beta), vp(scratch), nbytes, B, n, PREC[mode], 0, stream()]
    if feat:
        cf_g = gs.copy(cf.cuda(), "oi_sdf_mlp_bwd_feat input g_feat")
        ok(L.oi_sdf_mlp_bwd_feat(*[vp(t) for t in ins], vp(cf_g), *outs), "oi_sdf_mlp_bwd_feat")
    else:
        ok(L.oi_sdf_mlp_bwd(*[vp(t) for t in ins], *outs), "oi_sdf_mlp_bwd")
    got = _unpack_bwd(d_small, d_wmat)
    got["w"] = _d_w_from_film(P, d_gamma, d_beta, range(9))
    bad = {k: rel_err(v, ref[k]) for k, v in got.items() if rel_err(v, ref[k]) > 2e-5}
    assert not bad, bad
    # the padding floats of d_small stay as the caller cleared them
    assert float(d_small[1665:1668].abs().max()) == 0.0 and float(d_small[2439].abs()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. colour head and lattice
# ---------------------------------------------------------------------------------------------------------------------
# bars: tests/test_gpu_kernels.py::test_color_network_forward_standalone_golden_f2 (2e-5) and
#       tests/test_gpu_backward.py::COLOR_HEAD_BWD_TOL (5e-6 relative)
@pytest.mark.parametrize("npe", [1, 127, 129])
def test_color_head_ragged(guarded_ops, packs, col_sd, npe):
    L = _L()
    gs = guarded_ops
    P, _ = packs
    B = 3
    n = B * npe
    gen = torch.Generator().manual_seed(npe)
    feat = torch.rand(n, 128, generator=gen) * 2 - 1
    nrm = torch.randn(n, 3, generator=gen) * 3
    w = torch.randn(B, 64, generator=gen)
    c = torch.randn(n, 3, generator=gen)
    csd = {k: v.double().requires_grad_(True) for k, v in col_sd.items()}
    fo, no, wo = (t.double().requires_grad_(True) for t in (feat, nrm, w))
    rgb_o = O.color_head(csd, fo, no, wo)
    g_o = dict(zip(["feat", "normals", "w"] + list(csd), torch.autograd.grad((rgb_o * c.double()).sum(), [fo, no, wo] + list(csd.values()))))
    gamma, beta = _film(P, w)
    gam, bet = gamma[:, 8].contiguous(), beta[:, 8].contiguous()
    heads = [gs.copy(col_sd[k].cuda().contiguous(), "colour head " + k) for k in
             ("views_linears.weight", "views_linears.bias", "rgb_linear.weight", "rgb_linear.bias")]
    fg, ng, gg, bg_, cg = (gs.copy(t.cuda(), "colour head input") for t in (feat, nrm, gam, bet, c))
    rgb = gs.empty((n, 3), torch.float32, "cuda", "oi_color_head_fwd rgb")
    ok(L.oi_color_head_fwd(vp(fg), vp(ng), vp(gg), vp(bg_), 128, *[vp(h) for h in heads], vp(rgb), B, npe, stream()),
       "oi_color_head_fwd")
    assert maxdiff(rgb.cpu(), rgb_o) < 2e-5
    ws_bytes = L.oi_color_head_bwd_workspace_bytes(B, npe)
    ws = gs.scratch(ws_bytes, "cuda", "oi_color_head_bwd workspace")
    o = {k: gs.empty(s, torch.float32, "cuda", "oi_color_head_bwd " + k) for k, s in
         (("feat", (n, 128)), ("normals", (n, 3)), ("gamma", (B, 128)), ("beta", (B, 128)), ("views_linears.weight", (128, 131)),
          ("views_linears.bias", (128,)), ("rgb_linear.weight", (3, 128)), ("rgb_linear.bias", (3,)))}
    ok(L.oi_color_head_bwd(vp(fg), vp(ng), vp(gg), vp(bg_), 128, *[vp(h) for h in heads], vp(cg), vp(o["feat"]), vp(o["normals"]),
                           vp(o["gamma"]), vp(o["beta"]), 128, vp(o["views_linears.weight"]), vp(o["views_linears.bias"]),
                           vp(o["rgb_linear.weight"]), vp(o["rgb_linear.bias"]), vp(ws), ws_bytes, B, npe, stream()),
       "oi_color_head_bwd")
    got = {k: o[k] for k in ("feat", "normals") + tuple(k for k in o if "linear" in k)}
    got["w"] = _d_w_from_film(P, o["gamma"][:, None].expand(B, 9, 128), o["beta"][:, None].expand(B, 9, 128), [8])
    bad = {k: rel_err(v, g_o[k]) for k, v in got.items() if rel_err(v, g_o[k]) > 5e-6}
    assert not bad, bad


# bar: tests/test_gpu_mesh.py (bit-identical to the sdf path; 1e-4 of the oracle)
@pytest.mark.parametrize("B,res", [(1, (2, 2, 2)), (2, (3, 5, 7)), (1, (129, 2, 3))])
def test_sdf_lattice_small_and_ragged(guarded_ops, packs, sdf_sd, B, res):
    L = _L()
    gs = guarded_ops
    P, pk = packs
    nx, ny, nz = res
    axes = [torch.linspace(-0.9, 0.8, k) for k in res]
    g = torch.Generator().manual_seed(sum(res) + B)
    w = O.style_mlp(sdf_sd, torch.randn(B, 64, generator=g))
    gamma, beta = _film(P, w)
    xs, ys, zs = (gs.copy(a.cuda(), "oi_sdf_lattice axis") for a in axes)
    out = gs.empty((B, nx, ny, nz), torch.float32, "cuda", "oi_sdf_lattice out")
    ok(L.oi_sdf_lattice(vp(gs.copy(pk["f16x3"], "packed")), vp(gs.copy(gamma, "gamma")), vp(gs.copy(beta, "beta")), B, vp(xs),
                        vp(ys), vp(zs), nx, ny, nz, ctypes.c_float(-1.0), vp(out), PREC["f16x3"], 0, stream()), "oi_sdf_lattice")
    X, Y, Z = torch.meshgrid(*axes, indexing="ij")
    pts = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], -1)
    ref = _mlp_fwd_guarded(gs, pts.repeat(B, 1), pk["f16x3"], gamma, beta, B, pts.shape[0], "f16x3", False, False, False)[0]
    assert torch.equal(out.reshape(-1), -ref)
    for b in range(B):
        sd_b = O.sdf_forward({k: v.double() for k, v in sdf_sd.items()}, pts.double(), w[b:b + 1].double())[0].reshape(res)
        assert maxdiff(out[b].cpu(), -sd_b) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 4. render chain
# ---------------------------------------------------------------------------------------------------------------------
def _rays(N, seed):
    g = torch.Generator().manual_seed(seed)
    ro = torch.tensor([0.0, 0.0, -3.0]).expand(N, 3) + 0.05 * torch.randn(N, 3, generator=g)
    rd = F.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(N, 3, generator=g), dim=-1)
    near, far = O.near_far_from_sphere(ro, rd)
    return ro.contiguous(), rd.contiguous(), near, far, g


@pytest.mark.parametrize("R", [1, 3])
def test_gen_rays_small(guarded_ops, R):
    """oi_gen_rays / oi_gen_rays_light at R = 1 and 3 against the fp64 pinhole rays of oracle.gen_rays (generator.py:255-279):
    pixel (i, j) -> p = kinv (offs_x + j R / (R - 1), offs_y + i R / (R - 1), 1) (linspace(0, 1, R) scaled by R; 0 at R = 1),
    rays_d = c2b[:3, :3] p / |p|, rays_o = c2b[:3, 3]; near / far of those rays.  Bars of tests/test_gpu_kernels.py::test_gen_rays
    (origins / near / far 1e-5, directions 2e-6)."""
    from oi_amd import ops
    B = 2
    g = torch.Generator().manual_seed(R)
    q = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=torch.float64)).Q
    c2b = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    c2b[:, :3, :3] = q
    c2b[:, :3, 3] = -2.5 * q[:, :, 2]
    c2b = c2b.float()
    kinv = torch.tensor([[0.01, 0.0, -0.5], [0.0, 0.012, -0.45], [0.0, 0.0, 1.0]])
    offs = torch.tensor([[30.0, 40.0], [47.0, 3.0]])
    lin = torch.linspace(0, 1, R, dtype=torch.float64) * R
    px = (lin[None, None, :] + offs[:, 0, None, None].double()).expand(B, R, R)
    py = (lin[None, :, None] + offs[:, 1, None, None].double()).expand(B, R, R)
    p = torch.stack([px, py, torch.ones_like(px)], -1) @ kinv.double().t()
    rd_o = torch.einsum("bij,bhwj->bhwi", c2b[:, :3, :3].double(), p / p.norm(dim=-1, keepdim=True))
    ro_o = c2b[:, None, None, :3, 3].double().expand_as(rd_o)
    ldir = torch.tensor([0.3, -0.5, -0.8])
    args = [gs_copy(guarded_ops, t) for t in (c2b, kinv, offs)]
    ro, rd, near, far = ops.gen_rays(*args, R)
    ro2, rd2, near2, far2, ld = ops.gen_rays(*args, R, w2b=gs_copy(guarded_ops, c2b), light_direction=gs_copy(guarded_ops, ldir))
    for a, b in ((ro, ro2), (rd, rd2), (near, near2), (far, far2)):
        assert torch.equal(a, b)
    assert maxdiff(ro.cpu(), ro_o) < 1e-5 and maxdiff(rd.cpu(), rd_o) < 2e-6
    n_o, f_o = O.near_far_from_sphere(ro_o.reshape(-1, 3), rd_o.reshape(-1, 3))
    assert maxdiff(near.cpu(), n_o) < 1e-5 and maxdiff(far.cpu(), f_o) < 1e-5
    d = ldir.double()
    assert maxdiff(ld.cpu(), c2b[:, :3, :3].double() @ (d / d.norm())) < 1e-5


def test_coarse_samples_and_midpoints_single_sample(guarded_ops):
    """S = T = 1 (oi_coarse_samples, oi_midpoints): z = near (torch.linspace(0, 1, 1) == [0]), dists = last_dist."""
    from oi_amd import ops
    N = 5
    ro, rd, near, far, g = _rays(N, 1)
    jit = torch.rand(N, 1, generator=g)
    for j in (None, jit):
        z, pts = ops.coarse_samples(*(gs_copy(guarded_ops, t) for t in (ro, rd, near, far)), 1,
                                    None if j is None else gs_copy(guarded_ops, j))
        z_o = near if j is None else near + (j - 0.5) * 2.0
        assert maxdiff(z.cpu(), z_o) < 1e-6
        assert maxdiff(pts.cpu(), ro[:, None] + rd[:, None] * z_o[..., None]) < 1e-6
    dists, mid, pts = ops.midpoints(gs_copy(guarded_ops, ro), gs_copy(guarded_ops, rd), gs_copy(guarded_ops, z), 2.0)
    assert maxdiff(dists.cpu(), torch.full((N, 1), 2.0)) == 0 and maxdiff(mid.cpu(), z.cpu() + 1.0) < 1e-6


def _up_inputs(N, Sc, seed):
    ro, rd, near, far, g = _rays(N, seed)
    z = torch.sort(near + (far - near) * torch.rand(N, Sc, generator=g), -1).values
    pts = ro[:, None] + rd[:, None] * z[..., None]
    sdf = (0.5 - pts.norm(dim=-1)) + 0.01 * torch.randn(N, Sc, generator=g)   # a sphere: weight concentrated near its surface
    return ro, rd, z.contiguous(), sdf.contiguous(), g


# bars: tests/test_gpu_kernels.py::test_upsample_vs_oracle (z_new 5e-5; merge exact)
@pytest.mark.parametrize("Sc,n_new", [(2, 1), (2, 1024), (63, 65), (1024, 1), (1024, 1024)])
def test_upsample_and_merge_up_to_max_sc(guarded_ops, Sc, n_new):
    """oi_upsample (Sc and n_new up to MAX_SC = 1024) and oi_merge_sorted, ties included."""
    from oi_amd import ops
    N = 5
    ro, rd, z, sdf, g = _up_inputs(N, Sc, Sc + n_new)
    inv_s = 64.0
    wts = O.up_sample_weights(ro.double(), rd.double(), z.double(), sdf.double(), inv_s)
    zn_o = O.sample_pdf_det(z.double(), wts, n_new)
    z_new, pts_new, z_m = ops.upsample(*(gs_copy(guarded_ops, t) for t in (ro, rd, z, sdf)), n_new, inv_s)
    assert maxdiff(z_new.cpu(), zn_o) < 5e-5
    assert torch.equal(z_m.cpu(), torch.sort(torch.cat([z, z_new.cpu()], -1), -1).values)
    assert maxdiff(pts_new.cpu(), ro[:, None] + rd[:, None] * z_new.cpu()[..., None]) < 1e-6
    # merge with ties: every other new z equals an existing one; the sdf is a function of z, so equal z carry equal sdf
    # and the order of a tie cannot change the result
    z_t = z_new.cpu().clone()
    pick = torch.randint(0, Sc, (N, n_new), generator=g)
    z_t[:, ::2] = torch.gather(z, 1, pick)[:, ::2]
    z_t = torch.sort(z_t, -1).values
    s_m, s_t = torch.sin(37.0 * z), torch.sin(37.0 * z_t)
    zo, so = ops.merge_sorted(*(gs_copy(guarded_ops, t) for t in (z, s_m, z_t, s_t)))
    zr, sr = O.merge_sorted(z, z_t, s_m, s_t)
    assert torch.equal(zo.cpu(), zr) and torch.equal(so.cpu(), sr)


# 5. the > 64 KiB dynamic-LDS launch of oi_upsample_mid: bit-identical to oi_upsample + oi_midpoints (include/oi_hip.h), and
#    within the bar of tests/test_gpu_kernels.py::test_upsample_vs_oracle
@pytest.mark.parametrize("Sc,n_new", [(1024, 1024), (700, 650)])
def test_upsample_mid_large_lds(guarded_ops, Sc, n_new):
    from oi_amd import ops
    assert 4 * (4 * Sc + 2 * n_new) * 4 > 64 * 1024
    N = 9
    ro, rd, z, sdf, _ = _up_inputs(N, Sc, Sc * 3 + n_new)
    ins = [gs_copy(guarded_ops, t) for t in (ro, rd, z, sdf)]
    a = ops.upsample(*ins, n_new, 128.0, merge=True)
    d_a = ops.midpoints(ins[0], ins[1], a[2], 2.0 / Sc)
    b = ops.upsample(*ins, n_new, 128.0, mid_last_dist=2.0 / Sc)
    for x, y in zip(list(a) + list(d_a), list(b[:3]) + list(b[3])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # (the oracle in fp32, as in test_upsample_vs_oracle: with 700+ bins the inverse CDF of nearly empty sections amplifies the
    # fp32 rounding of the cumulative sum, which that bar was set against)
    wts = O.up_sample_weights(ro, rd, z, sdf, 128.0)
    assert maxdiff(b[0].cpu(), O.sample_pdf_det(z, wts, n_new)) < 5e-5


def _composite_ref(sdf, grad, rgb, dists, mid_z, ro, rd, inv_s, car):
    """fp64 restatement of oracle.render_core's compositing on given per-sample values."""
    N, T = sdf.shape
    dirs = rd[:, None, :].expand(N, T, 3)
    true_cos = (dirs * grad).sum(-1)
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - car) + F.relu(-true_cos) * car)
    prev = torch.sigmoid((sdf - iter_cos * dists * 0.5) * inv_s)
    nxt = torch.sigmoid((sdf + iter_cos * dists * 0.5) * inv_s)
    alpha = ((prev - nxt + 1e-5) / (prev + 1e-5)).clamp(0.0, 1.0)
    weights = O.transmittance_weights(alpha)
    pn = (ro[:, None, :] + rd[:, None, :] * mid_z[..., None]).norm(dim=-1)
    return {"weights": weights, "cdf": prev, "alpha": alpha, "inside_sphere": (pn < 1.0).double(), "pts_norm": pn,
            "weight_sum": weights.sum(-1, keepdim=True), "weight_max": weights.max(-1, keepdim=True)[0],
            "color_fine": (rgb * weights[..., None]).sum(1)}


# bars: tests/test_gpu_kernels.py::test_composite_vs_oracle_maps (per-sample 1e-5, maps 2e-5)
@pytest.mark.parametrize("N,B", [(1, 1), (3, 3), (5, 1), (6, 2)])
@pytest.mark.parametrize("T", [1, 63, 65, 2048])
def test_composite_ragged(guarded_ops, N, B, T):
    """oi_composite_fwd (block partials sized by oi_composite_num_blocks) + oi_render_stats, and oi_composite_bwd."""
    from oi_amd import ops
    g = torch.Generator().manual_seed(N * 10000 + T)
    ro, rd, near, far, _ = _rays(N, N + T)
    z = torch.sort(near + (far - near) * torch.rand(N, T, generator=g), -1).values
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), 2.0 / max(T, 2))], -1)
    mid = z + 0.5 * dists
    pts = ro[:, None] + rd[:, None] * mid[..., None]
    sdf = 0.6 - pts.norm(dim=-1)
    grad = -F.normalize(pts, dim=-1) + 0.1 * torch.randn(N, T, 3, generator=g)
    rgb = torch.rand(N, T, 3, generator=g)
    var = torch.tensor(0.3)
    light = torch.tensor([-0.4, 0.35, 6.0])
    ldir = torch.randn(B, 3, generator=g)
    bg = torch.rand(B, 3, generator=g)
    car = 0.37
    ins = [gs_copy(guarded_ops, t) for t in (sdf, grad, rgb, dists, mid, ro, rd, ldir, bg, var, light)]
    out = ops.composite_fwd(*ins[:11], car, B)
    inv_s = float(O.inv_s_from_variance(var.double()))
    ref = _composite_ref(*(t.double() for t in (sdf, grad, rgb, dists, mid, ro, rd)), inv_s, car)
    for k in ("weights", "cdf", "alpha", "pts_norm"):
        assert maxdiff(out[k].cpu(), ref[k]) < 1e-5, k
    assert maxdiff(out["inside_sphere"].cpu(), ref["inside_sphere"]) == 0
    for k in ("weight_sum", "weight_max", "color_fine"):
        assert maxdiff(out[k].cpu(), ref[k]) < 2e-5, k
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    # oi_render_stats (the default two-launch form): the block reductions at ragged N, against the restatement
    pn = ref["pts_norm"]
    relax = (pn < 1.2).double()
    gnorm = grad.double().norm(dim=-1)
    r4_o = torch.stack([(relax * (gnorm - 1.0) ** 2).sum(), relax.sum(), torch.exp(-100.0 * sdf.double().abs()).sum()])
    sums_o = torch.stack([ref["cdf"][:, 0].sum(), ref["weight_max"].sum(), ref["weight_sum"].sum()])
    fin_o = torch.stack([r4_o[0] / (r4_o[1] + 1e-5), r4_o[2] / (N * T), *(sums_o / N)])
    for got, want in ((out["reduce4"][:3], r4_o), (out["ray_sums"][:3], sums_o), (out["finals"], fin_o)):
        assert maxdiff(got.cpu(), want) < 2e-5 * max(1.0, float(want.abs().max())), (got, want)
    # the one-launch form (its last workgroup sums the partials: stats16 + ticket) is bit-identical to it
    ops.FUSED_STATS = True
    try:
        out_f = ops.composite_fwd(*ins[:11], car, B)
    finally:
        ops.FUSED_STATS = False
    for k in ("reduce4", "ray_sums", "finals", "weights", "image"):
        assert torch.equal(out_f[k], out[k]), k
    # backward through the same inputs (at most T = 1280 samples: include/oi_hip.h oi_composite_bwd): every per-sample gradient
    # written, against fp64 autograd of the restatement
    if T > 1280:
        T = 1280
        sdf, grad, rgb, dists, mid = (t[:, :T].contiguous() for t in (sdf, grad, rgb, dists, mid))
        ins = [gs_copy(guarded_ops, t) for t in (sdf, grad, rgb, dists, mid)] + ins[5:]
    gw = torch.randn(N, T, generator=g)
    gc = torch.randn(N, 3, generator=g)
    gs_ = torch.randn(N, 1, generator=g)
    d_sdf, d_grad, d_rgb, d_var, d_light, d_ldir = ops.composite_bwd(*ins[:11], car, B, {
        "weights": gs_copy(guarded_ops, gw), "color_fine": gs_copy(guarded_ops, gc), "weight_sum": gs_copy(guarded_ops, gs_)})
    sd, gd, cd = (t.double().requires_grad_(True) for t in (sdf, grad, rgb))
    vd = var.double().requires_grad_(True)
    r = _composite_ref(sd, gd, cd, *(t.double() for t in (dists, mid, ro, rd)), O.inv_s_from_variance(vd), car)
    loss = (r["weights"] * gw.double()).sum() + (r["color_fine"] * gc.double()).sum() + (r["weight_sum"] * gs_.double()).sum()
    e_sdf, e_grad, e_rgb, e_var = torch.autograd.grad(loss, [sd, gd, cd, vd])
    for a, b in ((d_sdf, e_sdf), (d_grad, e_grad), (d_rgb, e_rgb)):
        assert maxdiff(a.cpu(), b) < 2e-5 * max(1.0, float(b.abs().max()))
    # d_variance is a sum over all N x T samples: the bar of tests/test_gpu_backward.py::test_composite_backward_vs_oracle
    # (COMPOSITE_BWD_TOL), relative to max(1, |d_variance|) as the other scalars here -- at N = 1 the samples' terms cancel
    # to ~1e-3 and a bar relative to that remainder alone would measure the cancellation, not the kernel
    assert abs(float(d_var) - float(e_var)) < 1.2e-3 * max(1.0, abs(float(e_var))), (float(d_var), float(e_var))
    # the light block and direction only reach the Phong maps, which carry no upstream gradient here
    assert not bool(d_light.any()) and not bool(d_ldir.any())


def gs_copy(gs, t):
    return gs.copy(t.float().contiguous().cuda(), "input")


# ---------------------------------------------------------------------------------------------------------------------
# 6. marching cubes (oi_mc_workspace_bytes, oi_mc_count, oi_mc_emit) against tests/helpers/mc_numpy.py
# ---------------------------------------------------------------------------------------------------------------------
def _mc_guarded(gs, u, iso, nv=None, nt=None):
    L = _L()
    nx, ny, nz = u.shape
    field = gs.copy(torch.from_numpy(u).cuda(), "oi_mc field")
    nbytes = L.oi_mc_workspace_bytes(nx, ny, nz)
    ws = gs.scratch(nbytes, "cuda", "oi_mc workspace")
    tot = (ctypes.c_longlong * 3)()
    ok(L.oi_mc_count(vp(field), nx, ny, nz, ctypes.c_float(iso), vp(ws), nbytes, tot, stream()), "oi_mc_count")
    nv = tot[0] if nv is None else nv
    nt = tot[1] if nt is None else nt
    v = gs.empty((nv, 3), torch.float32, "cuda", f"oi_mc_emit vertices[{nv}]")
    t = gs.empty((nt, 3), torch.int32, "cuda", f"oi_mc_emit triangles[{nt}]")
    ok(L.oi_mc_emit(vp(field), nx, ny, nz, ctypes.c_float(iso), vp(ws), nbytes, vp(v), nv, vp(t), nt, stream()), "oi_mc_emit")
    return (tot[0], tot[1]), v, t


def _ellipsoid(shape, radii, quantise=False):
    g = [np.arange(k, dtype=np.float64) for k in shape]
    X, Y, Z = np.meshgrid(*g, indexing="ij")
    c = [(k - 1) / 2 for k in shape]
    r = np.sqrt(((X - c[0]) / radii[0]) ** 2 + ((Y - c[1]) / radii[1]) ** 2 + ((Z - c[2]) / radii[2]) ** 2)
    u = 4.0 * (1.0 - r)
    return (np.round(u) if quantise else u).astype(np.float32)


# bar: tests/test_gpu_mesh.py::test_gpu_marching_cubes_matches_numpy (triangles equal, vertices 1e-6)
@pytest.mark.parametrize("name", ["1280_chunks", "threshold_ties"])
def test_marching_cubes_many_chunks_and_ties(guarded_ops, name):
    if name == "1280_chunks":   # 1024 x 80 x 64 = 1280 chunks of 4096 points: mc_scan_kernel gives threads more than one chunk
        u, iso = _ellipsoid((1024, 80, 64), (480.0, 36.0, 28.0)), 0.0
    else:                       # integer-valued field: many lattice values exactly equal to the threshold
        u, iso = _ellipsoid((40, 33, 47), (15.0, 12.0, 19.0), quantise=True), 1.0
        assert int((u == iso).sum()) > 100
    (nv, nt), v, t = _mc_guarded(guarded_ops, u, iso)
    vr, tr = M.marching_cubes(u, iso)
    assert (nv, nt) == (len(vr), len(tr)) and nt > 100
    assert np.array_equal(t.cpu().numpy().astype(np.int64), tr)
    assert float(np.abs(v.cpu().numpy() - vr).max()) <= 1e-6


def test_marching_cubes_emit_truncated(guarded_ops):
    """oi_mc_emit with n_vertices / n_triangles below the totals: exactly that prefix of the full mesh, nothing after it (the
    guard after each output starts at its last byte + 1)."""
    u = _ellipsoid((50, 41, 37), (20.0, 16.0, 15.0))
    (nv, nt), v, t = _mc_guarded(guarded_ops, u, 0.0)
    for kv, kt in ((nv // 2, nt // 3), (1, 1), (nv - 1, nt - 1)):
        _, v2, t2 = _mc_guarded(guarded_ops, u, 0.0, kv, kt)
        assert torch.equal(v2.view(torch.int32), v[:kv].view(torch.int32)) and torch.equal(t2, t[:kt])


# ---------------------------------------------------------------------------------------------------------------------
# 7. discriminator family, against fp64 torch
# ---------------------------------------------------------------------------------------------------------------------
# bars: tests/test_gpu_kernels.py::test_conv4x4_vs_torch (2e-5) / tests/test_gpu_backward.py::test_conv_dgrad_wgrad_vs_torch
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [4, 9])
@pytest.mark.parametrize("Cin", [1, 3, 5])
@pytest.mark.parametrize("Cout", [1, 7])
def test_conv4x4_family_small(guarded_ops, B, H, Cin, Cout):
    """Through oi_amd.ops (accumulate-outputs poisoned: the launcher must clear them): oi_conv4x4_fwd_arena,
    oi_conv4x4_dgrad_masked, oi_conv4x4_wgrad_masked, oi_conv4x4_bwd_pre, oi_conv4x4_dgrad_pre; then the plain entries."""
    from oi_amd import ops
    for stride, pad in ((2, 1), (1, 0)):
        g = torch.Generator().manual_seed(B + 10 * H + 100 * Cin + 1000 * Cout + stride)
        x = torch.randn(B, Cin, H, H, generator=g)
        w = torch.randn(Cout, Cin, 4, 4, generator=g) / math.sqrt(Cin * 16)
        b = torch.randn(Cout, generator=g)
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        pre = F.conv2d(F.leaky_relu(xd, 0.2), wd, None, stride=stride, padding=pad)
        y_ref = F.leaky_relu(pre + b.double()[None, :, None, None], 0.2)
        y = ops.conv4x4_fwd(gs_copy(guarded_ops, x), gs_copy(guarded_ops, w), gs_copy(guarded_ops, b), stride, pad, 0.2, x_slope=0.2)
        assert maxdiff(y.cpu(), y_ref) < 2e-5
        gy = torch.randn(pre.shape, generator=g)
        ref = F.leaky_relu(pre.detach(), 0.2)     # the producing layer's output: its LeakyReLU masks the incoming gradient
        g_eff = torch.where(ref > 0, gy.double(), 0.2 * gy.double())
        gx_pre, gw_o = torch.autograd.grad(pre, [xd, wd], g_eff)
        gx_plain = torch.nn.grad.conv2d_input(x.shape, wd.detach(), g_eff, stride=stride, padding=pad)
        gyc, refc, wc, xc = (gs_copy(guarded_ops, t) for t in (gy, ref, w, x))
        gx1 = ops.conv4x4_dgrad(gyc, wc, H, H, stride, pad, mask_ref=refc, slope=0.2)
        assert maxdiff(gx1.cpu(), gx_plain) < 2e-5
        gw_plain = torch.nn.grad.conv2d_weight(x.double(), w.shape, g_eff, stride=stride, padding=pad)
        gw1 = ops.conv4x4_wgrad(gyc, xc, stride, pad, mask_ref=refc, slope=0.2)
        assert maxdiff(gw1.cpu(), gw_plain) < 2e-5 * max(1.0, float(gw_plain.abs().max()))
        gx2, gw2 = ops.conv4x4_bwd(gyc, wc, xc, stride, pad, mask_ref=refc, slope=0.2)          # oi_conv4x4_bwd_pre, x_slope 1
        assert maxdiff(gx2.cpu(), gx_plain) < 2e-5 and maxdiff(gw2.cpu(), gw_plain) < 2e-5 * max(1.0, float(gw_plain.abs().max()))
        gx3, gw3 = ops.conv4x4_bwd(gyc, wc, xc, stride, pad, mask_ref=refc, slope=0.2, x_slope=0.2)
        assert maxdiff(gx3.cpu(), gx_pre) < 2e-5 and maxdiff(gw3.cpu(), gw_o) < 2e-5 * max(1.0, float(gw_o.abs().max()))
        gx4 = ops.conv4x4_dgrad_pre(gs_copy(guarded_ops, g_eff), wc, xc, 0.2, stride, pad)   # oi_conv4x4_dgrad_pre
        assert maxdiff(gx4.cpu(), gx_pre) < 2e-5
        # the plain entry points: oi_conv4x4_fwd / oi_conv4x4_fwd_into (y cleared by the launcher / by the caller),
        # oi_conv4x4_dgrad, oi_conv4x4_wgrad, oi_conv4x4_bwd_masked (accumulate = 0)
        L = _L()
        gs = guarded_ops
        Ho = (H + 2 * pad - 4) // stride + 1
        xg, bg_ = gs_copy(gs, x), gs_copy(gs, b)
        y_plain = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad), 0.2)
        y1 = gs.empty((B, Cout, Ho, Ho), torch.float32, "cuda", "oi_conv4x4_fwd y")
        ok(L.oi_conv4x4_fwd(vp(xg), vp(wc), vp(bg_), vp(y1), B, Cin, H, H, Cout, stride, pad, ctypes.c_float(0.2), stream()),
           "oi_conv4x4_fwd")
        y2 = gs.zeros((B, Cout, Ho, Ho), torch.float32, "cuda", "oi_conv4x4_fwd_into y")
        ok(L.oi_conv4x4_fwd_into(vp(xg), vp(wc), vp(bg_), vp(y2), B, Cin, H, H, Cout, stride, pad, ctypes.c_float(0.2),
                                 ctypes.c_float(1.0), 1, stream()), "oi_conv4x4_fwd_into")
        assert maxdiff(y1.cpu(), y_plain) < 2e-5 and maxdiff(y2.cpu(), y_plain) < 2e-5
        ge = gs_copy(gs, g_eff)
        gx5 = gs.empty(x.shape, torch.float32, "cuda", "oi_conv4x4_dgrad gx")
        ok(L.oi_conv4x4_dgrad(vp(ge), vp(wc), vp(gx5), B, Cin, H, H, Cout, stride, pad, stream()), "oi_conv4x4_dgrad")
        gw5 = gs.empty(w.shape, torch.float32, "cuda", "oi_conv4x4_wgrad gw")
        ok(L.oi_conv4x4_wgrad(vp(ge), vp(xc), vp(gw5), B, Cin, H, H, Cout, stride, pad, stream()), "oi_conv4x4_wgrad")
        gx6 = gs.empty(x.shape, torch.float32, "cuda", "oi_conv4x4_bwd_masked gx")
        gw6 = gs.empty(w.shape, torch.float32, "cuda", "oi_conv4x4_bwd_masked gw")
        ok(L.oi_conv4x4_bwd_masked(vp(gyc), vp(refc), ctypes.c_float(0.2), vp(wc), vp(xc), vp(gx6), vp(gw6), 0, B, Cin, H, H, Cout,
                                   stride, pad, stream()), "oi_conv4x4_bwd_masked")
        wtol = 2e-5 * max(1.0, float(gw_plain.abs().max()))
        for a_, b_, t_ in ((gx5, gx_plain, 2e-5), (gw5, gw_plain, wtol), (gx6, gx_plain, 2e-5), (gw6, gw_plain, wtol)):
            assert maxdiff(a_.cpu(), b_) < t_


@pytest.mark.parametrize("B,C,H", [(1, 1, 5), (3, 2, 9)])
def test_image_ops_small(guarded_ops, B, C, H):
    """oi_upfirdn2d, oi_affine_grid_sample_fwd, oi_affine_grid_sample_bwd, oi_reflect_pad_fwd, oi_reflect_pad_bwd,
    oi_fused_bias_act, oi_channel_sum,
    oi_lrelu_mask_mul on ragged small images against fp64 torch / the oracle (bars 1e-5 .. 2e-5 of their existing tests)."""
    from oi_amd import ops
    L = _L()
    gs = guarded_ops
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, C, H, H + 1, generator=g)
    f = torch.randn(4, 3, generator=g)
    y = ops.upfirdn2d(gs_copy(gs, x), gs_copy(gs, f), upx=2, upy=1, downx=1, downy=2, padx0=2, padx1=1, pady0=1, pady1=2)
    y_o = O.upfirdn2d(x.double(), f.double(), up=(2, 1), down=(1, 2), pad=(2, 1, 1, 2))
    assert y.shape == y_o.shape and maxdiff(y.cpu(), y_o) < 2e-5
    theta = torch.tensor([[[0.9, 0.1, 0.05], [-0.1, 1.1, -0.02]]]).repeat(B, 1, 1)
    ys = ops.affine_grid_sample_fwd(gs_copy(gs, x), gs_copy(gs, theta), H + 2, H - 1)
    grid = F.affine_grid(theta.double(), (B, C, H + 2, H - 1), align_corners=False)
    xd = x.double().requires_grad_(True)
    ys_o = F.grid_sample(xd, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    assert maxdiff(ys.cpu(), ys_o) < 2e-5
    gy = torch.randn(ys.shape, generator=g)
    gx = ops.affine_grid_sample_bwd(gs_copy(gs, gy), gs_copy(gs, theta), H, H + 1)
    assert maxdiff(gx.cpu(), torch.autograd.grad(ys_o, xd, gy.double())[0]) < 2e-5
    yp = ops.reflect_pad_fwd(gs_copy(gs, x), 2, 1, 1, 3)
    xp = x.double().requires_grad_(True)
    yp_o = F.pad(xp, (2, 1, 1, 3), mode="reflect")
    assert maxdiff(yp.cpu(), yp_o) == 0
    gp = torch.randn(yp.shape, generator=g)
    gxp = ops.reflect_pad_bwd(gs_copy(gs, gp), H, H + 1, 2, 1, 1, 3)
    assert maxdiff(gxp.cpu(), torch.autograd.grad(yp_o, xp, gp.double())[0]) < 1e-5
    cs = ops.channel_sum(gs_copy(gs, x))
    assert maxdiff(cs.cpu(), x.double().sum((0, 2, 3))) < 1e-5
    ref = torch.randn(x.shape, generator=g)
    lm = ops.lrelu_mask_mul(gs_copy(gs, x), gs_copy(gs, ref), 0.2)
    assert maxdiff(lm.cpu(), torch.where(ref > 0, x, 0.2 * x)) == 0
    bias = torch.randn(C, generator=g)
    out = gs.empty(x.shape, torch.float32, "cuda", "oi_fused_bias_act out")
    ok(L.oi_fused_bias_act(vp(out), vp(gs_copy(gs, x)), vp(gs_copy(gs, bias)), None, 3, 0, ctypes.c_float(0.2),
                           ctypes.c_float(math.sqrt(2.0)), x.numel(), H * (H + 1), C, stream()), "oi_fused_bias_act")
    fb = F.leaky_relu(x.double() + bias.double()[None, :, None, None], 0.2) * math.sqrt(2.0)
    assert maxdiff(out.cpu(), fb) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 8. multi-tensor optimiser steps (oi_multi_adam, oi_multi_rmsprop, oi_multi_lerp, oi_multi_copy)
# ---------------------------------------------------------------------------------------------------------------------
def _table(quads, chunk):
    rows = []
    for p, g, s0, s1 in quads:
        n = p.numel()
        for off in range(0, n, chunk):
            m = min(chunk, n - off)
            rows.append([p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, 0 if s0 is None else s0.data_ptr() + 4 * off,
                         0 if s1 is None else s1.data_ptr() + 4 * off, m])
    return torch.tensor(rows, dtype=torch.int64).cuda(), len(rows)


# bars: tests/test_gpu_modules.py::test_fused_optimizer_matches_torch (parameters 2e-7, state 1e-6, relative to max(1, |x|))
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind", ["adam", "rmsprop", "lerp", "copy"])
def test_multi_tensor_steps_chunk_edges(guarded_ops, kind, packed):
    L = _L()
    gs = guarded_ops
    c = L.oi_mt_chunk_elems()
    sizes = [1, c - 1, c, c + 1, 3 * c + 5]
    g = torch.Generator().manual_seed(len(kind) + packed)
    host = [[torch.randn(n, generator=g) for _ in range(4)] for n in sizes]
    for h in host:
        h[3] = h[3].abs()                     # exp_avg_sq / square_avg are non-negative
        if kind == "rmsprop":
            h[2] = h[2].abs()
    if packed:
        # all tensors back to back in ONE guarded buffer with 7-float sentinels between them that no chunk covers
        total = sum(4 * n + 4 * 7 for n in sizes)
        flat = gs.zeros((total,), torch.float32, "cuda", f"oi_multi_{kind} packed buffer")
        flat.copy_(torch.randn(total, generator=g))
        before = flat.clone()
        views, off, covered = [], 0, torch.zeros(total, dtype=torch.bool)
        for n, h in zip(sizes, host):
            quad = []
            for t in h:
                v = flat[off:off + n]
                v.copy_(t.cuda())
                covered[off:off + n] = True
                quad.append(v)
                off += n + 7
            views.append(quad)
    else:
        views = []
        for n, h in zip(sizes, host):
            quad = []
            for j, t in enumerate(h):
                v = gs.zeros((n,), torch.float32, "cuda", f"oi_multi_{kind} tensor[{n}] #{j}")
                v.copy_(t.cuda())
                quad.append(v)
            views.append(quad)
    quads = [(q[0], q[1], q[2] if kind in ("adam", "rmsprop") else None, q[3] if kind == "adam" else None) for q in views]
    table, rows = _table(quads, c)
    lr, b1, b2, eps, step = 1e-3, 0.5, 0.9, 1e-8, 3
    bc1, bc2s = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
    if kind == "adam":
        ok(L.oi_multi_adam(vp(table), rows, ctypes.c_float(lr), ctypes.c_float(b1), ctypes.c_float(b2), ctypes.c_float(1 - b1),
                           ctypes.c_float(1 - b2), ctypes.c_float(eps), ctypes.c_float(bc1), ctypes.c_float(bc2s), stream()), "oi_multi_adam")
    elif kind == "rmsprop":
        ok(L.oi_multi_rmsprop(vp(table), rows, ctypes.c_float(lr), ctypes.c_float(0.99), ctypes.c_float(1 - 0.99), ctypes.c_float(eps),
                              stream()),
           "oi_multi_rmsprop")
    elif kind == "lerp":
        ok(L.oi_multi_lerp(vp(table), rows, ctypes.c_float(0.999), stream()), "oi_multi_lerp")
    else:
        ok(L.oi_multi_copy(vp(table), rows, stream()), "oi_multi_copy")
    for (p0, g0, s0, s1), (p, _, a, b) in zip(host, quads):
        p0, g0, s0, s1 = (t.double() for t in (p0, g0, s0, s1))
        if kind == "adam":
            m = b1 * s0 + (1 - b1) * g0
            v = b2 * s1 + (1 - b2) * g0 * g0
            pe = p0 - lr / bc1 * m / (v.sqrt() / bc2s + eps)
            assert maxdiff(a.cpu(), m) <= 1e-6 * max(1.0, float(m.abs().max()))
            assert maxdiff(b.cpu(), v) <= 1e-6 * max(1.0, float(v.abs().max()))
        elif kind == "rmsprop":
            s = 0.99 * s0 + 0.01 * g0 * g0
            pe = p0 - lr * g0 / (s.sqrt() + eps)
            assert maxdiff(a.cpu(), s) <= 1e-6 * max(1.0, float(s.abs().max()))
        elif kind == "lerp":
            pe = g0 + 0.999 * (p0 - g0)
        else:
            pe = g0
        assert maxdiff(p.cpu(), pe) <= 2e-7 * max(1.0, float(pe.abs().max())), (kind, p.numel())
    if packed:
        assert torch.equal(flat.cpu()[~covered], before.cpu()[~covered]), "a sentinel between two tensors changed"


# ---------------------------------------------------------------------------------------------------------------------
# 9. small ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_small_ops(guarded_ops, B):
    """oi_light_dir_fwd, oi_light_dir_bwd, oi_render_scalars_fwd, oi_render_scalars_bwd, oi_weighted_sum_fwd,
    oi_weighted_sum_bwd, oi_gan_losses_fwd, oi_gan_losses_bwd, oi_stage_inputs, oi_scalar_glue, oi_zero_fill against fp64
    restatements of their contracts (include/oi_hip.h)."""
    from oi_amd import ops
    gs = guarded_ops
    g = torch.Generator().manual_seed(B)
    d = torch.randn(3, generator=g)
    w2b = torch.eye(4).repeat(B, 1, 1)
    w2b[:, :3, :3] = torch.linalg.qr(torch.randn(B, 3, 3, generator=g)).Q
    dd = d.double().requires_grad_(True)
    n_o = F.normalize(w2b[:, :3, :3].double() @ F.normalize(dd, dim=0), dim=-1)
    n = ops.light_dir_fwd(gs_copy(gs, d), gs_copy(gs, w2b))
    assert maxdiff(n.cpu(), n_o) < 1e-6
    gn = torch.randn(B, 3, generator=g)
    gd = ops.light_dir_bwd(gs_copy(gs, d), gs_copy(gs, w2b), gs_copy(gs, gn))
    assert maxdiff(gd.cpu(), torch.autograd.grad(n_o, dd, gn.double())[0]) < 1e-5
    r4 = torch.rand(4, generator=g) + 0.5
    o2 = ops.render_scalars_fwd(gs_copy(gs, r4), 0.125)
    assert maxdiff(o2.cpu(), torch.stack([r4[0].double() / (r4[1].double() + 1e-5), r4[2].double() * 0.125])) < 1e-6
    ge, gsf = torch.tensor([0.7]), torch.tensor([-1.3])
    g4 = ops.render_scalars_bwd(gs_copy(gs, r4), gs_copy(gs, ge), gs_copy(gs, gsf), 0.125)
    r = r4.double()
    g4_o = torch.tensor([0.7 / (r[1] + 1e-5), -0.7 * r[0] / (r[1] + 1e-5) ** 2, -1.3 * 0.125, 0.0], dtype=torch.float64)
    assert maxdiff(g4.cpu(), g4_o) < 1e-6 * max(1.0, float(g4_o.abs().max()))
    terms = [gs_copy(gs, torch.randn(1, generator=g)) for _ in range(B + 2)]
    wts = [0.5 * (i + 1) for i in range(B + 2)]
    tot = ops.weighted_sum_fwd(terms, wts)
    assert abs(float(tot) - sum(w * float(t) for w, t in zip(wts, terms))) < 1e-6 * max(1.0, abs(float(tot)))
    gt = ops.weighted_sum_bwd(gs_copy(gs, torch.tensor([2.0])), wts, "cuda")
    assert maxdiff(gt.cpu(), 2.0 * torch.tensor(wts, dtype=torch.float64)) == 0
    K = 4
    dr, df, pose = (torch.randn(B, K, generator=g), torch.randn(B, K, generator=g), torch.randn(B, K - 1, generator=g))
    gx = torch.randn(B, 5, generator=g)
    aux = torch.tensor([0.3])
    out6 = ops.gan_losses_fwd(*(gs_copy(gs, t) for t in (dr, df, pose, gx, aux)), 10.0)
    real = F.binary_cross_entropy_with_logits(dr[:, 0].double(), torch.ones(B, dtype=torch.float64))
    fake = F.binary_cross_entropy_with_logits(df[:, 0].double(), torch.zeros(B, dtype=torch.float64))
    reg = (gx.double() ** 2).sum(1).mean()
    auxl = ((df[:, 1:].double() - pose.double()) ** 2).mean()
    o6 = torch.stack([real + fake + 10 * reg + 0.3 * auxl, real + fake, reg, fake, real, auxl])
    assert maxdiff(out6.cpu(), o6) < 1e-5 * max(1.0, float(o6.abs().max()))
    g_r, g_f, g_x = ops.gan_losses_bwd(gs_copy(gs, torch.tensor([1.0])), *(gs_copy(gs, t) for t in (dr, df, pose, gx, aux)), 10.0,
                                       True, True, True)
    drd, dfd, gxd = (t.double().requires_grad_(True) for t in (dr, df, gx))
    tot_o = (F.binary_cross_entropy_with_logits(drd[:, 0], torch.ones(B, dtype=torch.float64))
             + F.binary_cross_entropy_with_logits(dfd[:, 0], torch.zeros(B, dtype=torch.float64))
             + 10 * (gxd ** 2).sum(1).mean() + 0.3 * ((dfd[:, 1:] - pose.double()) ** 2).mean())
    for a, b in zip((g_r, g_f, g_x), torch.autograd.grad(tot_o, [drd, dfd, gxd])):
        assert maxdiff(a.cpu(), b) < 1e-6 * max(1.0, float(b.abs().max()))
    srcs = [gs_copy(gs, torch.randn(k, generator=g)) for k in (1, 5, 64 * B + 3)]
    dsts = [gs.empty((s.numel(),), torch.float32, "cuda", f"oi_stage_inputs dst[{s.numel()}]") for s in srcs]
    imm_dst = gs.empty((B + 60,), torch.float32, "cuda", "oi_stage_inputs imm_dst")
    imm = [float(i) * 0.25 for i in range(B + 60)]
    ops.stage_inputs(list(zip(srcs, dsts)), imm, imm_dst)
    for s, t in zip(srcs, dsts):
        assert torch.equal(s, t)
    assert maxdiff(imm_dst.cpu(), torch.tensor(imm)) == 0
    var, amb, spec, shin = (torch.tensor(v) for v in (0.3, -0.4, 0.35, 6.0))
    out5, packed3 = ops.scalar_glue(*(gs_copy(gs, t).reshape(()) for t in (var, amb, spec, shin)))
    inv_s = min(max(math.exp(10 * 0.3), 1e-6), 1e6)
    sa = 1 / (1 + math.exp(0.4))
    assert maxdiff(out5.cpu(), torch.tensor([inv_s, 1 / inv_s, sa, 1 - sa, 0.35], dtype=torch.float64)) < 1e-6 * inv_s
    assert maxdiff(packed3.cpu(), torch.tensor([-0.4, 0.35, 6.0])) == 0
    for n_z in (1, 63, 1000 + B):
        zf = gs.empty((n_z,), torch.float32, "cuda", f"oi_zero_fill[{n_z}]")
        ok(_L().oi_zero_fill(vp(zf), n_z, stream()), "oi_zero_fill")
        assert not bool(zf.view(torch.int32).any())


@pytest.mark.parametrize("mode", list(PREC))
def test_mlp_pack_weights_guarded(guarded_ops, packs, mode):
    """oi_mlp_pack_weights into a guarded buffer of exactly oi_mlp_packed_bytes(prec) bytes (guards only: the image may keep
    padding), bit-identical to the module's own image; oi_mlp_pack_status reads its header."""
    L = _L()
    gs = guarded_ops
    P, pk = packs
    nbytes = L.oi_mlp_packed_bytes(PREC[mode])
    out = gs.scratch(nbytes, "cuda", f"oi_mlp_pack_weights[{mode}] packed")
    args = [gs.copy(P[k].reshape(-1) if k in ("wsig", "bsig") else P[k], "pack input " + k)
            for k in ("w0", "b0", "wh", "bh", "wsig", "bsig", "wv", "bv", "wrgb", "brgb")]
    ok(L.oi_mlp_pack_weights(*[vp(a) for a in args], vp(out), PREC[mode], stream()), "oi_mlp_pack_weights")
    ok(L.oi_mlp_pack_status(vp(out), stream()), "oi_mlp_pack_status")
    assert out.numel() == pk[mode].numel()
    # the same image as the module's own pack, word for word -- up to the last bits of the f16x3 growth bounds, which are sums
    # formed with LDS atomics (order-dependent); every word the packer left out keeps the poison here
    a, b = out.view(torch.int32), pk[mode].view(torch.int32)
    diff = (a != b).nonzero().flatten()
    assert diff.numel() <= 16, diff.numel()
    fa, fb = out.view(torch.float32)[diff].double(), pk[mode].view(torch.float32)[diff].double()
    assert bool(((fa - fb).abs() <= 1e-5 * fb.abs()).all()), (diff.tolist(), fa.tolist(), fb.tolist())


# ---------------------------------------------------------------------------------------------------------------------
# 7b. discriminator forwards at ragged batches, augmentation, grid sampling, FiLM backward
# ---------------------------------------------------------------------------------------------------------------------
DISC_CHANS = [3, 64, 128, 256, 512]     # DCDiscriminator(img_size 64, n_feat 512), the network both fast paths cover
DISC_OUT = 7


@lru_cache(maxsize=None)
def _disc_weights():
    """Variance-preserving uniform weights (O(1) logits), as tests/test_gpu_modules.py::test_large_batch_discriminator_forward_vs_oracle."""
    g = torch.Generator().manual_seed(64)
    shapes = [(DISC_CHANS[i + 1], DISC_CHANS[i], 4, 4) for i in range(4)] + [(DISC_OUT, 512, 4, 4)]
    ws = [(torch.rand(s, generator=g) * 2 - 1) * (6.0 / (1.04 * s[1] * 16)) ** 0.5 for s in shapes]
    bias = torch.rand(DISC_OUT, generator=g) * 0.2 - 0.1
    return ws, bias


def _disc_ref(x, ws, bias):
    dsd = {f"blocks.{i}.weight": w.double() for i, w in enumerate(ws[:4])}
    dsd["conv_out.weight"], dsd["conv_out.bias"] = ws[4].double(), bias.double()
    return O.dc_discriminator(dsd, x.double())


# bar: tests/test_gpu_modules.py::test_large_batch_discriminator_forward_vs_oracle (2e-5 against the fp64 oracle)
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_disc_fwd_small_ragged_batch(guarded_ops, B):
    """oi_disc_fwd_small (workspace of exactly oi_disc_fwd_small_workspace_floats floats, OI_TICKET_WORDS ticket) at B = 1..4
    without augmentation, against the fp64 oracle; then the plan forms oi_disc_graph_launch_eager / oi_disc_graph_launch into
    guarded logits, bit-identical to it."""
    L = _L()
    gs = guarded_ops
    ws, bias = _disc_weights()
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(B))
    wg = [gs.copy(w.cuda(), f"disc weight {i}") for i, w in enumerate(ws)]
    bg_, xg = gs.copy(bias.cuda(), "disc bias"), gs.copy(x.cuda(), "disc x")
    n = L.oi_disc_fwd_small_workspace_floats(B, 3, 0, 0, 0, 0)
    wsp = gs.scratch(4 * n, "cuda", "oi_disc_fwd_small workspace")
    ticket = gs.zeros((4097,), torch.int32, "cuda", "oi_disc_fwd_small ticket")
    logits = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_fwd_small logits")
    ok(L.oi_disc_fwd_small(vp(xg), None, None, vp(xg), 0, 0, 0, 0, *[vp(w) for w in wg], vp(bg_), vp(wsp), vp(ticket), vp(logits),
                           B, 3, 64, 64, 512, DISC_OUT, ctypes.c_float(0.2), stream()), "oi_disc_fwd_small")
    assert maxdiff(logits.cpu(), _disc_ref(x, ws, bias)) < 2e-5
    assert not bool(ticket.any())                     # (the kernel leaves its arrival counters at zero)
    wsp2 = gs.scratch(4 * n, "cuda", "oi_disc_graph workspace")
    ticket2 = gs.zeros((4097,), torch.int32, "cuda", "oi_disc_graph ticket")
    plan_logits = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_graph logits")
    h = ctypes.c_void_p()
    ok(L.oi_disc_graph_create(ctypes.byref(h), 0, vp(xg), 0, 0, 0, 0, *[vp(w) for w in wg], vp(bg_), vp(wsp2), vp(ticket2),
                              vp(plan_logits), B, 3, 64, 64, 512, DISC_OUT, ctypes.c_float(0.2)), "oi_disc_graph_create")
    try:
        eager = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_graph_launch_eager logits")
        ok(L.oi_disc_graph_launch_eager(h, vp(xg), None, vp(eager), stream()), "oi_disc_graph_launch_eager")
        ok(L.oi_disc_graph_launch(h, vp(xg), None, stream()), "oi_disc_graph_launch")
        torch.cuda.synchronize()
        assert torch.equal(eager, logits) and torch.equal(plan_logits, logits)
    finally:
        L.oi_disc_graph_destroy(h)


@pytest.mark.parametrize("B", [1, 3])
def test_disc_plan_ada_draws_ragged_batch(guarded_ops, B):
    """oi_disc_graph_launch_ada (the library draws the matrices from a seed) into guarded logits: bit-identical to
    oi_disc_fwd_small given the same seed's matrices (oi_ada_theta_xint_scale) as host arrays (include/oi_hip.h)."""
    import oi_amd.augment as A
    L = _L()
    gs = guarded_ops
    ws, bias = _disc_weights()
    mx0, my0, mx1, my1 = (int(v) for v in A.AugmentPipe.static_margins(64, 64))
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(10 + B))
    wg = [gs.copy(w.cuda(), f"disc weight {i}") for i, w in enumerate(ws)]
    bg_, xg, f12 = gs.copy(bias.cuda(), "disc bias"), gs.copy(x.cuda(), "disc x"), gs.copy(O.hz_geom().cuda(), "f12")
    n = L.oi_disc_fwd_small_workspace_floats(B, 3, mx0, mx1, my0, my1)
    wsp = gs.scratch(4 * n, "cuda", "oi_disc_graph(ada) workspace")
    ticket = gs.zeros((4097,), torch.int32, "cuda", "oi_disc_graph(ada) ticket")
    plan_logits = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_graph(ada) logits (unused: eager)", must_write=False)
    h = ctypes.c_void_p()
    ok(L.oi_disc_graph_create(ctypes.byref(h), 1, vp(f12), mx0, mx1, my0, my1, *[vp(w) for w in wg], vp(bg_), vp(wsp),
                              vp(ticket), vp(plan_logits), B, 3, 64, 64, 512, DISC_OUT, ctypes.c_float(0.2)), "oi_disc_graph_create")
    try:
        seed, pars = 12345 + B, (1.0, 0.125, 1.0, 0.2)
        got = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_graph_launch_ada logits")
        ok(L.oi_disc_graph_launch_ada(h, vp(xg), seed, *pars, vp(got), 1, stream()), "oi_disc_graph_launch_ada")
        th = np.empty((B, 2, 3), np.float32)
        ok(L.oi_ada_theta_xint_scale(seed, B, 64, 64, mx0, mx1, my0, my1, *pars, th.ctypes.data_as(ctypes.c_void_p), None),
           "oi_ada_theta_xint_scale")
        n2 = L.oi_disc_fwd_small_workspace_floats(B, 3, mx0, mx1, my0, my1)
        wsp2 = gs.scratch(4 * n2, "cuda", "oi_disc_fwd_small(ada) workspace")
        ticket2 = gs.zeros((4097,), torch.int32, "cuda", "oi_disc_fwd_small(ada) ticket")
        ref = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_fwd_small(ada) logits")
        ok(L.oi_disc_fwd_small(vp(xg), th.ctypes.data_as(ctypes.c_void_p), None, vp(f12), mx0, mx1, my0, my1, *[vp(w) for w in wg],
                               vp(bg_), vp(wsp2), vp(ticket2), vp(ref), B, 3, 64, 64, 512, DISC_OUT, ctypes.c_float(0.2), stream()),
           "oi_disc_fwd_small")
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
    finally:
        L.oi_disc_graph_destroy(h)


@pytest.mark.parametrize("B", [16, 17, 24])
def test_disc_fwd_large_ragged_batch(guarded_ops, B):
    """oi_disc_large_pack into exactly oi_disc_large_packed_bytes (guards only) and oi_disc_fwd_large with a workspace of exactly
    oi_disc_large_workspace_bytes at B = 16, 17 (a ragged batch tail) and 24, against the fp64 oracle on EVERY image."""
    L = _L()
    gs = guarded_ops
    ws, bias = _disc_weights()
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(B))
    chans = (ctypes.c_int * 5)(*DISC_CHANS)
    wg = [gs.copy(w.cuda(), f"disc weight {i}") for i, w in enumerate(ws)]
    nbytes = L.oi_disc_large_packed_bytes(chans, 4, DISC_OUT)
    assert nbytes > 0
    packed = gs.scratch(nbytes, "cuda", "oi_disc_large_pack packed")
    ptrs = (ctypes.c_void_p * 4)(*[w.data_ptr() for w in wg[:4]])
    ok(L.oi_disc_large_pack(ptrs, vp(wg[4]), chans, 4, DISC_OUT, vp(packed), stream()), "oi_disc_large_pack")
    wbytes = L.oi_disc_large_workspace_bytes(chans, 4, DISC_OUT, B, 64)
    wsp = gs.scratch(wbytes, "cuda", "oi_disc_fwd_large workspace")
    logits = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_fwd_large logits")
    xg = gs.copy(x.cuda(), "disc x")
    ok(L.oi_disc_fwd_large(vp(xg), vp(wg[0]), vp(packed), vp(gs.copy(bias.cuda(), "disc bias")), vp(wsp), wbytes, vp(logits), chans,
                           4, DISC_OUT, B, 64, ctypes.c_float(0.2), stream()), "oi_disc_fwd_large")
    assert maxdiff(logits.cpu(), _disc_ref(x, ws, bias)) < 2e-5


# bar: tests/test_gpu_kernels.py::test_ada_geom_separable_matches_the_two_launch_form (2e-5 against the fp64 stages at 64 x 64)
@pytest.mark.parametrize("B,C", [(1, 1), (3, 3), (5, 2)])
def test_ada_geometry_small_batches(guarded_ops, B, C):
    """oi_ada_geom_sep_fwd / oi_ada_geom_sep_adj (one launch, axis-aligned matrices), oi_ada_geom_fwd (two launches, its canvas
    poisoned) and oi_ada_pad_up2 against the oracle's fp64 stages."""
    import oi_amd.augment as A
    from oi_amd import ops
    L = _L()
    gs = guarded_ops
    R = 64
    aug = A.AugmentPipe(xflip=1, xint=1, scale=1, aniso=1, xfrac=1).cuda()
    np.random.seed(B * 13 + C)
    x = torch.rand(B, C, R, R, generator=torch.Generator().manual_seed(B + C))
    G = aug.sample_G_inv(x.cuda())
    margins = aug.margins_for(G, R, R)
    mx0, my0, mx1, my1 = margins
    theta = torch.from_numpy(aug.theta_for(G, margins, R, R))
    f64 = aug.Hz_geom.double().cpu()
    xd = x.double().requires_grad_(True)
    xp = F.pad(xd, [mx0, mx1, my0, my1], mode="reflect")
    up = O.upsample2d(xp, f64)
    ref = O.downsample2d(O.affine_bilinear_sample(up, theta.double(), 2 * (R + 6), 2 * (R + 6)), f64, down=2, padding=-6, flip=True)
    f12, th_g, xg = gs.copy(aug.Hz_geom.float().cuda(), "f12"), gs.copy(theta.cuda(), "theta"), gs.copy(x.cuda(), "x")
    y_sep = ops.ada_geom_fwd(xg, th_g, f12, margins, axis_aligned=True)
    y_two = ops.ada_geom_fwd(xg, th_g, f12, margins, axis_aligned=False)
    assert maxdiff(y_sep.cpu(), ref) < 2e-5 and maxdiff(y_two.cpu(), ref) < 2e-5
    gy = torch.rand(B, C, R, R, generator=torch.Generator().manual_seed(1))
    gx = ops.ada_geom_adj_sep(gs.copy(gy.cuda(), "gy"), th_g, f12, margins)
    gx_o = torch.autograd.grad(ref, xd, gy.double())[0]
    assert maxdiff(gx.cpu(), gx_o) < 2e-5 * max(1.0, float(gx_o.abs().max()))
    canvas = gs.empty((B * C, 2 * (R + my0 + my1), 2 * (R + mx0 + mx1)), torch.float32, "cuda", "oi_ada_pad_up2 canvas")
    ok(L.oi_ada_pad_up2(vp(xg), vp(f12), vp(canvas), B, C, R, R, mx0, mx1, my0, my1, stream()), "oi_ada_pad_up2")
    assert maxdiff(canvas.cpu(), up.detach().reshape(canvas.shape)) < 2e-5


@pytest.mark.parametrize("N,C,Hi,Ho", [(1, 1, 5, 3), (3, 2, 9, 11)])
def test_grid_sample_small(guarded_ops, N, C, Hi, Ho):
    """oi_grid_sample_fwd / oi_grid_sample_bwd (gx and ggrid) into guarded outputs against fp64 torch (bilinear, zeros,
    align_corners=False; bar 2e-5 of the conv / resampling cases)."""
    L = _L()
    gs = guarded_ops
    g = torch.Generator().manual_seed(N * 10 + Hi)
    Wi, Wo = Hi + 2, Ho - 1
    x = torch.randn(N, C, Hi, Wi, generator=g)
    grid = torch.rand(N, Ho, Wo, 2, generator=g) * 2.4 - 1.2
    gy = torch.randn(N, C, Ho, Wo, generator=g)
    xd, gd = x.double().requires_grad_(True), grid.double().requires_grad_(True)
    y_o = F.grid_sample(xd, gd, mode="bilinear", padding_mode="zeros", align_corners=False)
    gx_o, gg_o = torch.autograd.grad(y_o, [xd, gd], gy.double())
    xg, gg_, gyg = (gs.copy(t.cuda(), "grid_sample input") for t in (x, grid, gy))
    y = gs.empty((N, C, Ho, Wo), torch.float32, "cuda", "oi_grid_sample_fwd y")
    ok(L.oi_grid_sample_fwd(vp(xg), vp(gg_), vp(y), N, C, Hi, Wi, Ho, Wo, stream()), "oi_grid_sample_fwd")
    gx = gs.empty(x.shape, torch.float32, "cuda", "oi_grid_sample_bwd gx")
    ggrid = gs.empty(grid.shape, torch.float32, "cuda", "oi_grid_sample_bwd ggrid")
    ok(L.oi_grid_sample_bwd(vp(gyg), vp(xg), vp(gg_), vp(gx), vp(ggrid), N, C, Hi, Wi, Ho, Wo, stream()), "oi_grid_sample_bwd")
    assert maxdiff(y.cpu(), y_o) < 2e-5 and maxdiff(gx.cpu(), gx_o) < 2e-5
    assert maxdiff(ggrid.cpu(), gg_o) < 2e-5 * max(1.0, float(gg_o.abs().max()))


# bar: tests/test_gpu_backward.py::test_film_params_backward_vs_oracle (2e-5 relative to max(1, |ref|))
@pytest.mark.parametrize("B", [1, 3])
def test_film_params_backward_small(guarded_ops, packs, sdf_sd, B):
    """oi_film_params_bwd through oi_amd.ops (every output guarded: assigned ones poisoned, accumulated ones zeroed) from z,
    against fp64 autograd of the style MLP + the nine FiLM heads (include/oi_hip.h oi_film_params)."""
    from oi_amd import ops
    P, _ = packs
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, 64, generator=g)
    dgam, dbet = torch.randn(B, 9, 128, generator=g), torch.randn(B, 9, 128, generator=g)
    st = {k: sdf_sd[k].double().requires_grad_(True) for k in sdf_sd if k.startswith("style.")}
    heads = {k: P[k].double().cpu().requires_grad_(True) for k in ("gw", "gb", "bw", "bb")}
    zd = z.double().requires_grad_(True)
    w = O.style_mlp(st, zd)
    gamma = 15.0 * (torch.einsum("bk,lfk->blf", w, heads["gw"]) + heads["gb"][None]) + 30.0
    beta = 0.25 * (torch.einsum("bk,lfk->blf", w, heads["bw"]) + heads["bb"][None])
    loss = (gamma * dgam.double()).sum() + (beta * dbet.double()).sum()
    names = list(heads) + ["style_w", "style_b", "z"]
    leaves = list(heads.values()) + [[st[f"style.{i}.weight"] for i in range(3)], [st[f"style.{i}.bias"] for i in range(3)], zd]
    flat = [t for l in leaves for t in (l if isinstance(l, list) else [l])]
    gr = torch.autograd.grad(loss, flat)
    ref = {"gw": gr[0], "gb": gr[1], "bw": gr[2], "bb": gr[3], "style_w": torch.stack(gr[4:7]), "style_b": torch.stack(gr[7:10]),
           "z": gr[10]}
    wf = ops.film_params(P["style_w"], P["style_b"], None, None, None, None, z=z.cuda())[0]
    out = ops.film_params_bwd(dgam.cuda(), dbet.cuda(), wf, P["gw"], P["bw"], P["style_w"], P["style_b"], z.cuda(), want_dz=True)
    for k in names:
        b = ref[k]
        a = out["d_" + k]
        assert maxdiff(a.cpu(), b) < 2e-5 * max(1.0, float(b.abs().max())), k


@pytest.mark.parametrize("B", [1, 3])
def test_disc_fwd_small128_ragged_batch(guarded_ops, B):
    """oi_disc_fwd_small128 (the shipped 128 x 128 / five-block network, workspace of exactly
    oi_disc_fwd_small128_workspace_floats floats) against the fp64 oracle, bar 2e-5 as above."""
    L = _L()
    gs = guarded_ops
    chans = [3, 32, 64, 128, 256, 512]
    g = torch.Generator().manual_seed(128 + B)
    shapes = [(chans[i + 1], chans[i], 4, 4) for i in range(5)] + [(DISC_OUT, 512, 4, 4)]
    ws = [(torch.rand(s, generator=g) * 2 - 1) * (6.0 / (1.04 * s[1] * 16)) ** 0.5 for s in shapes]
    bias = torch.rand(DISC_OUT, generator=g) * 0.2 - 0.1
    x = torch.rand(B, 3, 128, 128, generator=g)
    wg = [gs.copy(w.cuda(), f"disc128 weight {i}") for i, w in enumerate(ws)]
    xg = gs.copy(x.cuda(), "disc128 x")
    n = L.oi_disc_fwd_small128_workspace_floats(B, 3, 0, 0, 0, 0)
    wsp = gs.scratch(4 * n, "cuda", "oi_disc_fwd_small128 workspace")
    ticket = gs.zeros((4097,), torch.int32, "cuda", "oi_disc_fwd_small128 ticket")
    logits = gs.empty((B, DISC_OUT), torch.float32, "cuda", "oi_disc_fwd_small128 logits")
    ok(L.oi_disc_fwd_small128(vp(xg), None, None, vp(xg), 0, 0, 0, 0, *[vp(w) for w in wg], vp(gs.copy(bias.cuda(), "bias")), vp(wsp),
                              vp(ticket), vp(logits), B, 3, 512, DISC_OUT, ctypes.c_float(0.2), stream()), "oi_disc_fwd_small128")
    dsd = {f"blocks.{i}.weight": w.double() for i, w in enumerate(ws[:5])}
    dsd["conv_out.weight"], dsd["conv_out.bias"] = ws[5].double(), bias.double()
    assert maxdiff(logits.cpu(), O.dc_discriminator(dsd, x.double())) < 2e-5
