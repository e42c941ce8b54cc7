"""The style network and the FiLM heads (film_params_kernel, film_heads_bwd_kernel, style_bwd_kernel of csrc/mlp.hip; their copy
in prep_render_kernel of csrc/render.hip) and the stand-alone colour head (csrc/color_head.hip) against the float64 restatement
of tests/helpers/film_regimes.py in the regimes a trained model reaches.  Every bar is 3 x the committed float32 floor of its
(cell, tensor), at least 4 ulp of the tensor's largest entry and never above the project's existing bar
(tests/test_film_regimes_cpu.py); the measured errors go to film_regimes[...] of the margins file
(profiles/film_regimes_margins.txt)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, record_margin
from helpers import film_regimes as M
from helpers.guarded import POISON_WORD, guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]
NET_KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
ORDER_DEPENDENT = ("d_w", "d_style_w", "d_style_b", "d_z")    # atomics over layers / batch elements (d_z: through d_w)


def _bits_equal(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def _report(name, tensor, err):
    return f"{name}/{tensor}: error {err:.3e}, bar {M.bar(name, tensor):.3e}, float32 floor {M.FP32_FLOOR[M.canonical(name)][tensor]:.3e}"


def _judge(case, name, errs, bad):
    for tensor, err in errs.items():
        record_margin(f"film_regimes[{case}]", f"{name}/{tensor}", err)
        print(f"[{case}] {_report(name, tensor, err)}")
        if not err <= M.bar(name, tensor):
            bad.append(f"[{case}] {_report(name, tensor, err)}")


def _film_dev(c):
    return {k: c[k].cuda() for k in M.FILM_PARAMS}


def _film_forward(ops, c, P, nl=M.NL_ALL, l0=0):
    heads = [P[k][l0:l0 + nl] for k in ("gw", "gb", "bw", "bb")] if nl else [None] * 4
    if c["z"] is not None:
        return ops.film_params(P["style_w"], P["style_b"], *heads, z=c["z"].cuda())
    return ops.film_params(P["style_w"], P["style_b"], *heads, w=c["w"].cuda())


def _state_dicts(c):
    """The cell's style / head weights under the reference's state_dict names."""
    sd, csd = ({k: v.clone() for k, v in s.items()} for s in M.golden_sds())
    for i in range(3):
        sd[f"style.{i}.weight"], sd[f"style.{i}.bias"] = c["style_w"][i].clone(), c["style_b"][i].clone()
    for part, kw, kb in (("gamma", "gw", "gb"), ("beta", "bw", "bb")):
        for l in range(8):
            sd[f"pts_linears.{l}.{part}.weight"], sd[f"pts_linears.{l}.{part}.bias"] = c[kw][l].clone(), c[kb][l].clone()
        csd[f"views_linears.{part}.weight"], csd[f"views_linears.{part}.bias"] = c[kw][8].clone(), c[kb][8].clone()
    return sd, csd


def _prep_film(ops, P, z):
    """w, gamma, beta of ops.prep_render at the smallest R and S it accepts (1, 1), at most PREP_MAX_B elements per launch."""
    from oi_amd import lib
    outs = []
    for b0 in range(0, z.shape[0], lib.PREP_MAX_B):
        zs = z[b0:b0 + lib.PREP_MAX_B].contiguous()
        B = zs.shape[0]
        eye = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
        eye[:, 2, 3] = -3.0
        o = ops.prep_render(eye, eye, eye, np.zeros((B, 2), np.float32), np.zeros((B, 3), np.float32), torch.eye(3, device="cuda"),
                            1, 1, None, torch.tensor([0.3, -0.5, -0.8], device="cuda"), P, zs)
        outs.append((o["w"], o["gamma"], o["beta"]))
    return [torch.cat(x) for x in zip(*outs)]


@pytest.mark.parametrize("name", M.film_cells())
def test_film_forward_regime(name):
    """oi_film_params with all nine heads (z route, or the w route of `w_route`), with the eight sdf heads, the colour head alone
    and no head at all, FieldPack.film, and the copy inside the one-launch prep: w, gamma, beta finite and within the bars of
    the float64 restatement; the head subsets, FieldPack.film and prep_render bit for bit the nine-head call (csrc/render.hip
    promises "same operations in the same order")."""
    from oi_amd import ops
    from oi_amd.fields import ShapeNetwork, ColorNetwork, FieldPack
    c = M.cell(name)
    P = _film_dev(c)
    bad = []
    w, gamma, beta = _film_forward(ops, c, P)
    torch.cuda.synchronize()
    full = {"w": w, "gamma": gamma, "beta": beta}
    _judge("forward", name, M.errors(name, full), bad)
    # head counts: NL = 8 (sdf heads), NL = 1 (colour head), NL = 0 (style alone; the w route has nothing to run then)
    for nl, l0 in ((8, 0), (1, 8)) + (((0, 0),) if c["z"] is not None else ()):
        w2, g2, b2 = _film_forward(ops, c, P, nl, l0)
        assert _bits_equal(w2, w), f"{name}: w of the NL = {nl} call differs from the nine-head call"
        if nl:
            assert _bits_equal(g2, gamma[:, l0:l0 + nl]) and _bits_equal(b2, beta[:, l0:l0 + nl]), f"{name}: NL = {nl}, layers from {l0}"
        else:
            assert g2 is None and b2 is None
    # FieldPack.film: the modules' own route (stack cache, no-grad path)
    sd, csd = _state_dicts(c)
    sdf_net = ShapeNetwork(os.path.join(GOLDEN, "weights_sdf.npz"), **NET_KW)
    sdf_net.load_state_dict(sd)
    col_net = ColorNetwork(**NET_KW)
    col_net.load_state_dict(csd)
    pack = FieldPack(sdf_net.cuda(), col_net.cuda(), "f16x3")
    with torch.no_grad():
        wf, gf, bf = pack.film(z=c["z"].cuda()) if c["z"] is not None else pack.film(w=c["w"].cuda())
    _judge("FieldPack.film", name, M.errors(name, {"w": wf, "gamma": gf, "beta": bf}), bad)
    for k, v in (("w", wf), ("gamma", gf), ("beta", bf)):
        assert _bits_equal(v, full[k]), f"{name}: FieldPack.film's {k} differs from ops.film_params'"
    # the copy in prep_render_kernel (z route only: ops.prep_render takes latents)
    if c["z"] is not None:
        wp, gp, bp = _prep_film(ops, P, c["z"].cuda())
        _judge("prep_render", name, M.errors(name, {"w": wp, "gamma": gp, "beta": bp}), bad)
        for k, v in (("w", wp), ("gamma", gp), ("beta", bp)):
            d = v.view(torch.int32) != full[k].view(torch.int32)
            assert not bool(d.any()), f"{name}: {int(d.sum())} words of prep_render's {k} differ from oi_film_params', worst " \
                                      f"{float((v.double() - full[k].double()).abs().max()):.3e}"
    assert not bad, "; ".join(bad)


def _film_bwd(ops, c, P, w):
    kw = dict(style_w=P["style_w"], style_b=P["style_b"], z=c["z"].cuda(), want_dz=True) if c["z"] is not None else {}
    r = ops.film_params_bwd(c["cg"].cuda(), c["cb"].cuda(), w, P["gw"], P["bw"], d_w_in=c["cw"].cuda(), **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("name", M.film_cells(backward=True))
def test_film_backward_regime(name):
    """oi_film_params_bwd (heads + style, want_dz) and the style backward alone (ops.style_bwd, with and without d_z) against
    float64 autograd of <cg, gamma> + <cb, beta> + <cw, w>, per FiLM layer and per style layer.  layer_range: the layer whose
    cotangents are 0 gives exactly 0.  w_route: no style gradient exists.  Two calls: every output that no atomic touches is
    bit-identical (d_w is accumulated over the layers with atomics, d_style_w / d_style_b over the batch, and d_z is computed
    FROM d_w: those are held to the bar; with d_w fixed, ops.style_bwd's d_z is bit-identical too)."""
    from oi_amd import ops
    c = M.cell(name)
    P = _film_dev(c)
    w = _film_forward(ops, c, P)[0]
    r = _film_bwd(ops, c, P, w)
    got = M.split_film_grads(r)
    assert set(got) == set(M.film_backward_names(c)), sorted(set(got) ^ set(M.film_backward_names(c)))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f"{name}: {k} is not finite"
    bad = []
    _judge("backward", name, M.backward_errors(name, got), bad)
    r2 = M.split_film_grads(_film_bwd(ops, c, P, w))
    for k in got:
        if k.split(".")[0] not in ORDER_DEPENDENT:
            assert _bits_equal(got[k], r2[k]), f"{name}: {k} differs between two calls"
    _judge("backward(second call)", name, {k: v for k, v in M.backward_errors(name, r2).items() if k.split(".")[0] in ORDER_DEPENDENT}, bad)
    if c["regime"] == "layer_range":
        for k in ("d_gw", "d_gb", "d_bw", "d_bb"):
            v = got[f"{k}.{M.ZERO_COT_LAYER}"]
            assert int((v != 0).sum()) == 0, f"{k}[{M.ZERO_COT_LAYER}] has a zero cotangent and is not exactly 0: {float(v.abs().max()):.3e}"
    if c["z"] is None:
        assert not any(k.startswith("d_style") or k == "d_z" for k in r), sorted(r)
    else:
        # the style backward alone (NL = 0), from the d_w the heads left
        s1 = ops.style_bwd(r["d_w"], P["style_w"], P["style_b"], c["z"].cuda(), want_dz=True)
        s2 = ops.style_bwd(r["d_w"], P["style_w"], P["style_b"], c["z"].cuda(), want_dz=True)
        s3 = ops.style_bwd(r["d_w"], P["style_w"], P["style_b"], c["z"].cuda(), want_dz=False)
        torch.cuda.synchronize()
        assert "d_z" not in s3 and _bits_equal(s1["d_z"], s2["d_z"]) and _bits_equal(s1["d_z"], r["d_z"])
        for tag, s in (("style_bwd", s1), ("style_bwd(no d_z)", s3)):
            g = {f"{k}.{l}": s[k][l].cpu() for k in ("d_style_w", "d_style_b") for l in range(3)}
            if "d_z" in s:
                g["d_z"] = s["d_z"].cpu()
            _judge(tag, name, M.backward_errors(name, g), bad)
    assert not bad, "; ".join(bad)


# ----------------------------------------------------------------------------------------------------------------------
# the stand-alone colour head
# ----------------------------------------------------------------------------------------------------------------------
def _colour_dev(c):
    return [c[k].cuda() for k in M.COLOUR_LEAVES]


def _colour_run(ops, c):
    args = _colour_dev(c)
    rgb = ops.color_head_fwd(*args, c["B"])
    grads = ops.color_head_bwd(*args, c["cot"].cuda(), c["B"])
    torch.cuda.synchronize()
    return rgb, dict(zip(M.COLOUR_GRADS, grads))


def _colour_check(name):
    from oi_amd import ops
    c = M.cell(name)
    rgb, g = _colour_run(ops, c)
    assert bool(torch.isfinite(rgb).all()), f"{name}: rgb is not finite"
    for k, v in g.items():
        assert bool(torch.isfinite(v).all()), f"{name}: {k} is not finite"
    bad = []
    _judge("colour", name, M.errors(name, {"rgb": rgb}), bad)
    _judge("colour", name, M.backward_errors(name, g), bad)
    rgb2, g2 = _colour_run(ops, c)
    assert _bits_equal(rgb, rgb2), f"{name}: rgb differs between two calls"
    for k in g:
        assert _bits_equal(g[k], g2[k]), f"{name}: {k} differs between two calls (the file promises a fixed summation order)"
    assert not bad, "; ".join(bad)
    return c, rgb, g


@pytest.mark.parametrize("name", M.colour_cells())
def test_colour_head_regime(name):
    """oi_color_head_fwd / oi_color_head_bwd against float64 and its autograd; two calls bit-identical.  quiet_element: the
    element whose cotangent is 0 receives exactly 0 and adds nothing to the weight gradients.  saturated: everything finite,
    d_feat below its bar in absolute value.  The shape cells walk the chunk tails 1, 16, 17, 31, 32, 33 and five chunks."""
    from oi_amd import ops
    c, rgb, g = _colour_check(name)
    npe = c["npe"]
    if c["regime"] == "quiet_element":
        for k in ("d_gamma", "d_beta"):
            assert int((g[k][1] != 0).sum()) == 0, f"{k} of the quiet element: {float(g[k][1].abs().max()):.3e}"
        for k in ("d_feat", "d_normals"):
            assert int((g[k][npe:] != 0).sum()) == 0, f"{k} of the quiet element: {float(g[k][npe:].abs().max()):.3e}"
        one = [c[k][:npe].cuda() if k in ("feat", "normals") else c[k][:1].cuda() if k in ("gamma", "beta") else c[k].cuda()
               for k in M.COLOUR_LEAVES]
        alone = dict(zip(M.COLOUR_GRADS, ops.color_head_bwd(*one, c["cot"][:npe].cuda(), 1)))
        for k in ("d_wv", "d_bv", "d_wrgb", "d_brgb"):
            assert torch.equal(g[k], alone[k]), f"{k}: the quiet element changed it by {float((g[k] - alone[k]).abs().max()):.3e}"
    if c["regime"] == "saturated":
        assert float(g["d_feat"].abs().max()) <= M.bar(name, "d_feat"), float(g["d_feat"].abs().max())


def test_colour_head_chunks_larger_than_128():
    """B npe just above 131072: the point GEMM's chunks leave 128 points (160 here, 413 chunks per element, a tail of 80), the
    size every real caller runs at.  Once, on the trained_rgb weights."""
    name = f"colour/trained_rgb@{M.BIG_NPE}"
    cv = M.carve(M.COLOUR_B, M.BIG_NPE)
    assert cv["chunk_pts"] > 128 and cv["nchunk"] % 4 != 0
    _colour_check(name)


def test_colour_head_strides(guarded_ops):
    """gamma / beta read as layer 8 of a [B][9][128] tensor in place (film_stride = 1152) and d_gamma / d_beta written into
    layer 8 of a poisoned [B][9][128] tensor (d_film_stride = 1152), through the C ABI (oi_amd.ops always passes 128): bit for
    bit the stride-128 call, and the other eight layers keep their poison."""
    from oi_amd import lib, ops
    gs = guarded_ops
    L = lib.load()
    name = "colour/trained_rgb"
    c = M.cell(name)
    B, npe, n = c["B"], c["npe"], c["B"] * c["npe"]
    rgb_ref, g_ref = _colour_run(ops, c)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    layer8 = lambda t: ctypes.c_void_p(t.data_ptr() + 8 * M.C * 4)
    film = {}
    for k in ("gamma", "beta"):
        t = torch.full((B, M.NL_ALL, M.C), float("nan"))        # a row read from another layer poisons the result
        t[:, 8] = c[k]
        film[k] = gs.copy(t.cuda(), f"{k} [B][9][128]")
    feat, normals, wv, bv, wrgb, brgb, cot = (gs.copy(c[k].cuda(), k) for k in ("feat", "normals", "wv", "bv", "wrgb", "brgb", "cot"))
    rgb = gs.empty((n, 3), what="rgb (film_stride 1152)")
    lib.check(L.oi_color_head_fwd(p(feat), p(normals), layer8(film["gamma"]), layer8(film["beta"]), M.FILM_STRIDE_ALL, p(wv), p(bv),
                                  p(wrgb), p(brgb), p(rgb), B, npe, ops._stream()), "oi_color_head_fwd")
    out = {k: gs.empty(s, what=f"{k} (strided call)") for k, s in (("d_feat", (n, 128)), ("d_normals", (n, 3)), ("d_wv", (128, 131)),
                                                                    ("d_bv", (128,)), ("d_wrgb", (3, 128)), ("d_brgb", (3,)))}
    d_film = {k: gs.empty((B, M.NL_ALL, M.C), what=f"{k} [B][9][128]", must_write=False) for k in ("d_gamma", "d_beta")}
    ws_bytes = int(L.oi_color_head_bwd_workspace_bytes(B, npe))
    assert ws_bytes == M.carve(B, npe)["total"]
    ws = gs.scratch(ws_bytes, what="oi_color_head_bwd workspace")
    lib.check(L.oi_color_head_bwd(p(feat), p(normals), layer8(film["gamma"]), layer8(film["beta"]), M.FILM_STRIDE_ALL, p(wv), p(bv),
                                  p(wrgb), p(brgb), p(cot), p(out["d_feat"]), p(out["d_normals"]), layer8(d_film["d_gamma"]),
                                  layer8(d_film["d_beta"]), M.FILM_STRIDE_ALL, p(out["d_wv"]), p(out["d_bv"]), p(out["d_wrgb"]),
                                  p(out["d_brgb"]), p(ws), ws_bytes, B, npe, ops._stream()), "oi_color_head_bwd")
    torch.cuda.synchronize()
    assert _bits_equal(rgb, rgb_ref), "rgb with film_stride 1152 differs from the stride-128 call"
    for k, v in out.items():
        assert _bits_equal(v, g_ref[k]), f"{k} of the strided call differs from the stride-128 call"
    poison = int(np.uint32(POISON_WORD).astype(np.int32))
    for k, t in d_film.items():
        assert _bits_equal(t[:, 8], g_ref[k]), f"{k}: layer 8 of the stride-1152 tensor differs from the stride-128 call"
        rest = t[:, :8].contiguous().view(torch.int32)
        assert int((rest != poison).sum()) == 0, f"{k}: {int((rest != poison).sum())} words of the other eight layers were written"
    e = M.backward_errors(name, {k: d_film[k][:, 8] for k in d_film})
    for k, v in e.items():
        record_margin("film_regimes[colour, stride 1152]", f"{name}/{k}", v)
        assert v <= M.bar(name, k), _report(name, k, v)
